"""Differentiable marching tetrahedra (DMTet) on the HIP device: the front end of DiffSound's shape-fitting loops.

The reference runs marching tets as a few dozen torch ops with more than a dozen host synchronisations (boolean-mask
indexing, two ``torch.unique``, ``mask.sum()``) and a scipy graph pass for the connected component
(src/dmtet/geometry/dmtet_geometry.py:115-272 and :342-447, dmtet_thickness.py:99-200, dmtet_interpolate.py:115-205).
Here one engine (csrc/dmtet.hip) serves all three variants and returns the reference's outputs bit for bit:

* per grid, once: the unique edges (``ds_edge_table``), each tet's edge ids in DMTet's local order and a
  vertex -> incident-edge CSR (int32);
* per call: ``ds_mt_count`` (one count record read back: the only synchronisation), ``ds_mt_emit`` (vertices, tets,
  faces), and in the backward ``ds_mt_backward`` (gather over the CSR, no atomics).

``DMTet``, ``DMTetThickness`` and ``DMTetInterpolate`` take the reference classes' call signatures;
``DMTetGeometry`` is the reference's shape-fitting module (an MLP SDF on a deformable tet grid).
``DMTetThicknessGeometry`` and ``DMTetInterpolateGeometry`` are the ``DMTetGeometry`` classes of the reference's
dmtet_thickness.py and dmtet_interpolate.py: a fixed SDF on the grid, taken from a mesh file by
``diffsound_amd.meshsdf`` (the reference: open3d), with one learnable coefficient.
"""
import ctypes

import numpy as np
import torch
import torch.nn.functional as F

from . import _hip, meshgen, meshsdf
from .diffelastic.mesh import largest_connected_component

__all__ = ["marching_tets", "grid_tables", "kuhn_grid", "WeightedParam", "DMTet", "DMTetThickness", "DMTetInterpolate",
           "DMTetGeometry", "DMTetThicknessGeometry", "DMTetInterpolateGeometry", "TriangleMesh", "sdf_reg_loss", "PositionalEncoding", "NerfWithPositionEncoding",
           "largest_connected_component"]

# ds_edge_table's local edge order is (01)(12)(02)(03)(13)(23); DMTet's is [01, 02, 03, 12, 13, 23]
_EDGE_TABLE_TO_DMTET = [0, 2, 3, 1, 4, 5]


def _default_device():
    if not torch.cuda.is_available():
        raise RuntimeError("diffsound_amd.dmtet: no HIP device available (there is no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def kuhn_grid(res):
    """Jitter-free Kuhn grid of res^3 cells on [-0.5, 0.5]^3 (six tets per cell): (vertices (n,3) float32,
    indices (T,4) int64), the layout of the reference's data/tets/{res}_tets.npz files."""
    v, t = meshgen.kuhn_box(res, box=(1.0, 1.0, 1.0), jitter=0.0)
    return (v - np.float32(0.5)).astype(np.float32), t.astype(np.int64)


class GridTables:
    """The static tables of one tet grid on one device (int32): tets (T,4), tet_edge (T,6) in DMTet's local edge
    order, the distinct edges ea < eb sorted by (a, b), and the vertex -> incident-edge CSR (vptr, vadj)."""

    def __init__(self, tets, n):
        t64 = tets.long().contiguous()
        ea, eb, te = _hip.edge_table(t64, n)  # checks every index against [0, n)
        self.n, self.T, self.E = int(n), t64.shape[0], ea.shape[0]
        self.tets = t64.int().contiguous()
        self.tet_edge = te[:, _EDGE_TABLE_TO_DMTET].int().contiguous()
        self.ea, self.eb = ea.int().contiguous(), eb.int().contiguous()
        ends = torch.cat([ea, eb])
        ids = torch.arange(self.E, device=ea.device, dtype=torch.int32).repeat(2)
        self.vadj = ids[torch.argsort(ends, stable=True)].contiguous()
        cnt = torch.bincount(ends, minlength=self.n)
        self.vptr = torch.cat([cnt.new_zeros(1), torch.cumsum(cnt, 0)]).int().contiguous()
        self.count_ws = int(_hip.lib().ds_mt_count_workspace_bytes(self.n, self.T, self.E))
        if self.count_ws < 0:
            raise ValueError(f"marching_tets: grid too large (n={self.n}, T={self.T}, E={self.E})")


_TABLES = {}
_TABLES_CAP = 8


def grid_tables(tets, n):
    """GridTables of ``tets`` for an n-vertex grid, cached per (indices tensor, device).  The cache holds a reference
    to the indices tensor, so its storage (and the key) stays valid while the entry lives."""
    key = (tets.data_ptr(), tuple(tets.shape), tets.dtype, str(tets.device), tets._version, int(n))
    hit = _TABLES.get(key)
    if hit is not None:
        return hit[1]
    tab = GridTables(tets, n)
    if len(_TABLES) >= _TABLES_CAP:
        _TABLES.pop(next(iter(_TABLES)))
    _TABLES[key] = (tets, tab)
    return tab


def _check_inputs(pos, sdf, tets, band):
    if not isinstance(pos, torch.Tensor) or not isinstance(sdf, torch.Tensor) or not isinstance(tets, torch.Tensor):
        raise ValueError("marching_tets: pos, sdf and tets must be tensors")
    if not pos.is_cuda or pos.dtype != torch.float32 or pos.dim() != 2 or pos.shape[1] != 3 or pos.shape[0] == 0:
        raise ValueError("marching_tets: pos must be a non-empty (n, 3) float32 HIP tensor")
    n = pos.shape[0]
    if sdf.device != pos.device or sdf.dtype != torch.float32 or not (
            tuple(sdf.shape) == (n,) or tuple(sdf.shape) == (n, 1)):
        raise ValueError("marching_tets: sdf must be an (n,) or (n, 1) float32 tensor on pos's device")
    if tets.device != pos.device or tets.dtype not in (torch.int64, torch.int32) or tets.dim() != 2 or \
            tets.shape[1] != 4 or tets.shape[0] == 0:
        raise ValueError("marching_tets: tets must be a non-empty (T, 4) int64/int32 tensor on pos's device")
    if band is not None:
        if not isinstance(band, torch.Tensor):
            band = torch.tensor(float(band), dtype=torch.float32, device=pos.device)
        if band.numel() != 1 or band.dtype != torch.float32:
            raise ValueError("marching_tets: band must be a float32 scalar")
        if band.device != pos.device:
            band = band.to(pos.device)
    return band


class _MarchingTets(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pos, sdf, thick, tab, want_faces):
        dev = pos.device
        p = pos.contiguous()
        s = sdf.reshape(-1).contiguous()
        th = None if thick is None else thick.reshape(1).contiguous()
        n, T, E = tab.n, tab.T, tab.E
        toff = torch.empty((T, 5), dtype=torch.int32, device=dev)
        edge_id = torch.empty(E, dtype=torch.int32, device=dev)
        vert_id = torch.empty(n, dtype=torch.int32, device=dev)
        work = torch.empty(tab.count_ws, dtype=torch.uint8, device=dev)
        c = _hip.MtCounts()
        _hip.launch("ds_mt_count", s.data_ptr(), n, tab.tets.data_ptr(), T, tab.ea.data_ptr(), tab.eb.data_ptr(), E, tab.vptr.data_ptr(),
                    _hip.ptr(th), toff.data_ptr(), edge_id.data_ptr(), vert_id.data_ptr(), work.data_ptr(), tab.count_ws,
                    ctypes.byref(c), device=dev)
        nt = c.n_side1 + c.n_side3 + c.n_inner
        verts = torch.empty((c.n_used + c.n_cross, 3), dtype=torch.float32, device=dev)
        tets = torch.empty((nt, 4), dtype=torch.int64, device=dev)
        faces = torch.empty((c.n_face1 + c.n_face2 if want_faces else 0, 3), dtype=torch.int64, device=dev)
        vsrc = torch.empty(c.n_used, dtype=torch.int32, device=dev)
        xedge = torch.empty(c.n_cross, dtype=torch.int32, device=dev)
        _hip.launch("ds_mt_emit", p.data_ptr(), s.data_ptr(), n, tab.tets.data_ptr(), T, tab.tet_edge.data_ptr(), tab.ea.data_ptr(),
                    tab.eb.data_ptr(), E, tab.vptr.data_ptr(), _hip.ptr(th), toff.data_ptr(), edge_id.data_ptr(), vert_id.data_ptr(),
                    ctypes.byref(c), verts.data_ptr(), tets.data_ptr(), faces.data_ptr() if want_faces else None, vsrc.data_ptr(),
                    xedge.data_ptr(), device=dev)
        ctx.save_for_backward(p, s, th, edge_id, vert_id, xedge)
        ctx.tab, ctx.n_used, ctx.n_cross = tab, c.n_used, c.n_cross
        ctx.sdf_shape, ctx.thick_shape = sdf.shape, None if thick is None else thick.shape
        ctx.mark_non_differentiable(tets, faces)
        return verts, tets, faces, torch.tensor(c.n_used)

    @staticmethod
    def backward(ctx, gv, _gt, _gf, _gn):
        p, s, th, edge_id, vert_id, xedge = ctx.saved_tensors
        tab, n = ctx.tab, ctx.tab.n
        dev = p.device
        nout = ctx.n_used + ctx.n_cross
        gv = torch.zeros((nout, 3), dtype=torch.float32, device=dev) if gv is None else gv.contiguous().float()
        dpos = torch.empty((n, 3), dtype=torch.float32, device=dev)
        dsdf = torch.empty(n, dtype=torch.float32, device=dev)
        dt = work = None
        if th is not None:
            dt = torch.empty(1, dtype=torch.float32, device=dev)
            work, _ = _hip.workspace("ds_mt_backward_workspace_floats", ctx.n_cross, device=dev, dtype=torch.float32)
        _hip.launch("ds_mt_backward", gv.data_ptr() if nout else None, p.data_ptr(), s.data_ptr(), n, tab.ea.data_ptr(),
                    tab.eb.data_ptr(), tab.E, tab.vptr.data_ptr(), tab.vadj.data_ptr(), _hip.ptr(th), edge_id.data_ptr(),
                    vert_id.data_ptr(), xedge.data_ptr() if ctx.n_cross else None, ctx.n_used, ctx.n_cross, dpos.data_ptr(),
                    dsdf.data_ptr(), _hip.ptr(dt), _hip.ptr(work), device=dev)
        return dpos, dsdf.reshape(ctx.sdf_shape), None if dt is None else dt.reshape(ctx.thick_shape), None, None


def marching_tets(pos, sdf, tets, band=None, faces=False):
    """Differentiable marching tets of the SDF ``sdf`` ((n,) or (n, 1) float32) on the grid (``pos`` (n, 3) float32,
    ``tets`` (T, 4)), all on one HIP device.  Inside is ``sdf > 0``, or ``0 < sdf <= band`` when ``band`` (the
    thickness t, a float32 scalar tensor or a number) is given.

    Returns ``(verts, tets)``, the reference's ``all_verts_result, all_tets_result``; with ``faces=True``
    ``(verts, tets, surf_verts, faces)``, where ``surf_verts`` are the interpolated edge vertices (a view of the tail
    of ``verts``) and ``faces`` index them.  Gradients flow to ``pos``, ``sdf`` and ``band``."""
    band = _check_inputs(pos, sdf, tets, band)
    tab = grid_tables(tets, pos.shape[0])
    verts, tet_out, face_out, n_used = _MarchingTets.apply(pos, sdf, band, tab, bool(faces))
    if not faces:
        return verts, tet_out
    return verts, tet_out, verts[int(n_used):], face_out


class WeightedParam(torch.nn.Module):
    """A scalar in [min, max] of ``values_list`` as a softplus-weighted mean (the reference's
    src/dmtet/geometry/sdf.py WeightedParam: same parameter name and initialisation)."""

    def __init__(self, values_list):
        super().__init__()
        self.values_list = values_list
        self.probablity = torch.nn.Parameter(torch.zeros(len(values_list)))
        self.probablity.data.uniform_(-1, 1)

    def forward(self):
        probablity = F.softplus(self.probablity)
        probablity = probablity / probablity.sum()
        return (self.values_list.to(probablity.device) * probablity).sum()


class DMTet:
    """Plain marching tets, ``__call__(pos_nx3, sdf_n, tet_fx4) -> (verts, tets)`` (dmtet_geometry.py:20-272)."""

    def __call__(self, pos_nx3, sdf_n, tet_fx4):
        return marching_tets(pos_nx3, sdf_n, tet_fx4)


class DMTetThickness:
    """Hollow shell of thickness t: occupancy ``0 < sdf <= t`` with t = thickness_coef * max_thickness
    (dmtet_thickness.py:13-200).  ``__call__(pos_nx3, sdf_n, tet_fx4, thickness_coef=None) ->
    (verts, faces, all_verts_tetmesh, all_tets_tetmesh)``.  The caller sets ``max_thickness``, as in the reference."""

    def __init__(self):
        self.thickness_list = torch.linspace(0, 1, steps=32)
        self.thickness_coef = WeightedParam(self.thickness_list)

    def __call__(self, pos_nx3, sdf_n, tet_fx4, thickness_coef=None):
        if thickness_coef is None:
            thickness = self.thickness_coef() * self.max_thickness
        else:
            thickness = thickness_coef * self.max_thickness
        if not isinstance(thickness, torch.Tensor):
            thickness = torch.tensor(float(thickness), dtype=torch.float32)
        verts_all, tets_all, verts, faces = marching_tets(pos_nx3, sdf_n, tet_fx4, band=thickness.float(), faces=True)
        return verts, faces, verts_all, tets_all


class DMTetInterpolate:
    """Marching tets of the blend ``c * sdf1 + (1 - c) * sdf2`` (dmtet_interpolate.py:29-205).
    ``__call__(pos_nx3, sdf_n1, sdf_n2, tet_fx4, interp_coef=None) -> (verts, faces, all_verts, all_tets)``;
    ``sdf_n2 = None`` marches ``sdf_n1`` alone."""

    def __init__(self):
        self.interp_list = torch.linspace(0, 1, steps=32)
        self.interp_coef = WeightedParam(self.interp_list)

    def __call__(self, pos_nx3, sdf_n1, sdf_n2, tet_fx4, interp_coef=None):
        if sdf_n2 is None:
            sdf_n = sdf_n1
        else:
            if interp_coef is None:
                interp_coef = self.interp_coef()
            if isinstance(interp_coef, torch.Tensor):
                interp_coef = interp_coef.to(sdf_n1.device)
            sdf_n = interp_coef * sdf_n1 + (1 - interp_coef) * sdf_n2
        verts_all, tets_all, verts, faces = marching_tets(pos_nx3, sdf_n, tet_fx4, faces=True)
        return verts, faces, verts_all, tets_all


def sdf_reg_loss(sdf, all_edges):
    """Cross-entropy of the SDF signs across sign-changing grid edges (dmtet_geometry.py:280-293)."""
    sdf_f1x6x2 = sdf[all_edges.reshape(-1)].reshape(-1, 2)
    mask = torch.sign(sdf_f1x6x2[..., 0]) != torch.sign(sdf_f1x6x2[..., 1])
    sdf_f1x6x2 = sdf_f1x6x2[mask]
    if len(sdf_f1x6x2) == 0:
        return torch.tensor(0.0, device=sdf.device)
    return F.binary_cross_entropy_with_logits(sdf_f1x6x2[..., 0], (sdf_f1x6x2[..., 1] > 0).float()) + \
        F.binary_cross_entropy_with_logits(sdf_f1x6x2[..., 1], (sdf_f1x6x2[..., 0] > 0).float())


class PositionalEncoding(torch.nn.Module):
    """x -> [x, sin(2^i pi x / scale), cos(2^i pi x / scale) for i < freq_num] (dmtet_geometry.py:296-315)."""

    def __init__(self, freq_num=1, scale=1.0):
        super().__init__()
        self.freq_num = freq_num
        self.freqs = [2 ** i for i in range(freq_num)]
        self.scale = scale

    def forward(self, x):
        x_in = x
        for freq in self.freqs:
            x = torch.cat([x, torch.sin(freq * np.pi * x_in / self.scale), torch.cos(freq * np.pi * x_in / self.scale)],
                          dim=-1)
        return x


class NerfWithPositionEncoding(torch.nn.Module):
    """ReLU MLP on the positional encoding, one output (dmtet_geometry.py:318-339; same layer names and order)."""

    def __init__(self, freq_num=1, scale=1.0, layer_num=3, hidden_dim=256):
        super().__init__()
        self.freq_num = freq_num
        self.layer_num = layer_num
        self.hidden_dim = hidden_dim
        self.pos_enc = PositionalEncoding(freq_num, scale=scale)
        self.layer_0 = torch.nn.Linear(6 * freq_num + 3, hidden_dim)
        self.layers = torch.nn.ModuleList([torch.nn.Linear(hidden_dim, hidden_dim) for _ in range(layer_num)])
        self.final_layer = torch.nn.Linear(hidden_dim, 1)
        self.activation = F.relu

    def forward(self, x):
        x = self.activation(self.layer_0(self.pos_enc(x)))
        for layer in self.layers:
            x = self.activation(layer(x))
        return self.final_layer(x)


class DMTetGeometry(torch.nn.Module):
    """The reference's shape-fitting module (dmtet_geometry.py:342-447): an MLP SDF on a tet grid whose vertices move
    by at most 0.9 cell through ``deform``.  Loads ``data/tets/{res}_tets.npz`` from the working directory as the
    reference does, unless ``grid=(vertices, indices)`` is given.  Parameters are created in the reference's order
    (``state_dict`` round-trips both ways; one seed gives the same initial values); tensors live on the current HIP
    device."""

    def __init__(self, res, scale=1.0, freq_num=1, grid=None):
        super().__init__()
        dev = _default_device()
        self.scale = scale
        self.grid_res = res
        self.sdf_regularizer = 0.02
        self.marching_tets = DMTet()
        if grid is None:
            tets = np.load("data/tets/{}_tets.npz".format(self.grid_res))
            vertices, indices = tets["vertices"], tets["indices"]
        else:
            vertices, indices = grid
        self.base_verts = torch.as_tensor(np.asarray(vertices), dtype=torch.float32).to(dev)
        self.verts = self.base_verts * self.scale
        self.indices = torch.as_tensor(np.asarray(indices), dtype=torch.long).to(dev)
        self.generate_edges()
        self.sdf_nerf = NerfWithPositionEncoding(freq_num=freq_num, scale=scale, layer_num=3, hidden_dim=512)
        self.deform = torch.nn.Parameter(torch.zeros_like(self.verts), requires_grad=True)
        self.register_parameter("deform", self.deform)

    def mesh_template_loss(self, nodes, signed_distance, margin):
        sdf = self.sdf_nerf(nodes[signed_distance > margin])
        loss = 0
        return_none = True
        if len(sdf[sdf <= margin]) > 0:
            loss += -(sdf[sdf <= margin]).sum() / self.grid_res ** 3 * 1000
            return_none = False
        sdf = self.sdf_nerf(nodes[signed_distance < -margin])
        if len(sdf[sdf >= margin]) > 0:
            loss += (sdf[sdf >= margin]).sum() / self.grid_res ** 3 * 1000
            return_none = False
        if return_none:
            return None
        return loss

    def _deformed(self):
        return self.verts + self.scale * 1.8 / (self.grid_res * 2) * torch.tanh(self.deform)

    @property
    def sdf(self):
        return self.sdf_nerf(self._deformed() / self.scale)

    def generate_edges(self):
        """all_edges: the distinct grid edges (a < b), sorted (the reference's torch.unique of the sorted pairs)."""
        with torch.no_grad():
            ea, eb, _ = _hip.edge_table(self.indices, self.verts.shape[0])
            self.all_edges = torch.stack([ea, eb], dim=1)

    def getMesh(self):
        v_deformed = self._deformed()
        return self.marching_tets(v_deformed, self.sdf, self.indices)

    def get_largest_connected_component(self, verts, tets):
        return largest_connected_component(verts, tets)

    def reg_loss(self):
        return sdf_reg_loss(self.sdf, self.all_edges).mean() * self.sdf_regularizer


class TriangleMesh:
    """What ``getMesh(return_triangle=True)`` returns: the two fields of the reference's render.mesh.Mesh that the
    generate scripts' .obj export reads."""

    def __init__(self, v_pos, t_pos_idx):
        self.v_pos = v_pos
        self.t_pos_idx = t_pos_idx


def _summary_writer(FLAGS):
    """The reference's ``SummaryWriter(FLAGS.out_dir + "/tensorboard")`` unless FLAGS has ``without_tensorboard``.
    The one deviation: where the tensorboard package does not import, None (nothing is logged) instead of an
    ImportError at module import."""
    if hasattr(FLAGS, "without_tensorboard"):
        return None
    try:
        from torch.utils.tensorboard import SummaryWriter
    except ImportError:
        return None
    return SummaryWriter(FLAGS.out_dir + "/tensorboard")


class _MeshSdfGeometry(torch.nn.Module):
    """What the two classes below share (dmtet_thickness.py:204-248 and :298-326, dmtet_interpolate.py:209-262 and
    :303-360 are the same lines): the grid, its edges, the SDF of a mesh file at the grid vertices (positive inside)
    and the way from a marched tet mesh to a DiffSoundObj."""

    def __init__(self, grid_res, scale, FLAGS, grid=None):
        super().__init__()
        dev = _default_device()
        self.scale = scale
        self.FLAGS = FLAGS
        self.grid_res = grid_res
        writer = _summary_writer(FLAGS)
        if writer is not None:
            self.writer = writer
        if grid is None:
            tets = np.load("data/tets/{}_tets.npz".format(self.grid_res))
            vertices, indices = tets["vertices"], tets["indices"]
        else:
            vertices, indices = grid
        self.base_verts = torch.as_tensor(np.asarray(vertices), dtype=torch.float32).to(dev)
        self.verts = self.base_verts * self.scale
        self.indices = torch.as_tensor(np.asarray(indices), dtype=torch.long).to(dev)
        self.generate_edges()
        self.sdf = torch.zeros_like(self.verts[:, 0])

    def generate_edges(self):
        """all_edges: the distinct grid edges (a < b), sorted (the reference's torch.unique of the sorted pairs)."""
        with torch.no_grad():
            ea, eb, _ = _hip.edge_table(self.indices, self.verts.shape[0])
            self.all_edges = torch.stack([ea, eb], dim=1)

    @torch.no_grad()
    def getAABB(self):
        return torch.min(self.verts, dim=0).values, torch.max(self.verts, dim=0).values

    def get_largest_connected_component(self, verts, tets):
        return largest_connected_component(verts, tets)

    def _mesh_sdf(self, mesh_dir):
        """The SDF of the .obj file at the grid vertices, positive inside: the reference negates open3d's signed
        distance (dmtet_thickness.py:309-311)."""
        vertices, faces = meshsdf.read_obj(mesh_dir)
        signed_distance = meshsdf.MeshDistance(vertices, faces, device=self.verts.device).signed_distance(self.verts)
        return -signed_distance.reshape(-1)

    def _finish_mesh(self, marched, return_triangle):
        verts, faces, verts_tetmesh, tets_tetmesh = marched
        if return_triangle:
            return TriangleMesh(verts, faces)
        from .diffelastic.diff_model import DiffSoundObj
        from .diffelastic.material_model import MatSet

        verts_tetmesh, tets_tetmesh = self.get_largest_connected_component(verts_tetmesh, tets_tetmesh)
        mat = getattr(MatSet, self.FLAGS.mat) if hasattr(self.FLAGS, "mat") else MatSet.Ceramic
        return DiffSoundObj(verts_tetmesh, tets_tetmesh, mode_num=self.FLAGS.mode_num, order=self.FLAGS.order, mat=mat)

    def _audio_loss(self, target, it, name, coef):
        """tick's body: eigenvalue loss of the current mesh, printed and logged under ``name``."""
        sound_obj = self.getMesh()
        sound_obj.eigen_decomposition()
        vals = sound_obj.get_vals()
        audio_loss = ((vals - target) ** 2 / target ** 2).mean()
        print(name, coef().item(), "audio_loss", audio_loss.item())
        writer = getattr(self, "writer", None)
        if writer is not None:
            writer.add_scalar("loss", audio_loss.item(), it)
            writer.add_scalar(name, coef().item(), it)
        return audio_loss


class DMTetThicknessGeometry(_MeshSdfGeometry):
    """The reference's dmtet_thickness.DMTetGeometry (:203-326): the shell ``0 < sdf <= thickness_coef *
    max_thickness`` of a mesh file's SDF; the one parameter set is the thickness coefficient's.  Constructor
    ``(grid_res, scale, FLAGS)`` plus ``grid=(vertices, indices)`` in place of data/tets/{grid_res}_tets.npz."""

    def __init__(self, grid_res, scale, FLAGS, grid=None):
        super().__init__(grid_res, scale, FLAGS, grid=grid)
        self.marching_tets = DMTetThickness()

    def getMesh(self, return_triangle=False, thickness_coef=None):
        return self._finish_mesh(self.marching_tets(self.verts, self.sdf, self.indices, thickness_coef), return_triangle)

    def tick(self, target, it, FLAGS):
        return self._audio_loss(target, it, "thickness", self.marching_tets.thickness_coef)

    def apply_sdf(self, init_mesh_dir):
        self.sdf = self._mesh_sdf(init_mesh_dir)
        self.marching_tets.max_thickness = self.sdf.max()

    def parameters(self):
        return self.marching_tets.thickness_coef.parameters()

    def get_eigenvalues(self, thickness_coef=None):
        with torch.no_grad():
            sound_obj = self.getMesh(thickness_coef=thickness_coef)
            sound_obj.eigen_decomposition()
            vals = sound_obj.get_vals()
        return vals

    def get_thickness(self):
        return self.marching_tets.thickness_coef()


class DMTetInterpolateGeometry(_MeshSdfGeometry):
    """The reference's dmtet_interpolate.DMTetGeometry (:208-374): the blend ``c * sdf1 + (1 - c) * sdf2`` of two mesh
    files' SDFs (``apply_sdf2``), or one SDF alone (``apply_sdf`` with ``using_interp=False``); the one parameter set
    is the interpolation coefficient's.  Constructor as DMTetThicknessGeometry."""

    def __init__(self, grid_res, scale, FLAGS, grid=None):
        super().__init__(grid_res, scale, FLAGS, grid=grid)
        self.marching_tets = DMTetInterpolate()

    def getMesh(self, return_triangle=False, interp_coef=None, using_interp=True):
        if using_interp:
            marched = self.marching_tets(self.verts, self.sdf1, self.sdf2, self.indices, interp_coef)
        else:
            marched = self.marching_tets(self.verts, self.sdf, None, self.indices, interp_coef)
        return self._finish_mesh(marched, return_triangle)

    def tick(self, target, it, FLAGS):
        return self._audio_loss(target, it, "interp_coef", self.marching_tets.interp_coef)

    def apply_sdf(self, mesh_dir):
        self.sdf = self._mesh_sdf(mesh_dir)

    def apply_sdf2(self, mesh_dir1, mesh_dir2):
        self.sdf1 = self._mesh_sdf(mesh_dir1)
        self.sdf2 = self._mesh_sdf(mesh_dir2)

    def parameters(self):
        return self.marching_tets.interp_coef.parameters()

    def get_eigenvalues(self, interp_coef=None, using_interp=True):
        with torch.no_grad():
            sound_obj = self.getMesh(interp_coef=interp_coef, using_interp=using_interp)
            sound_obj.eigen_decomposition()
            vals = sound_obj.get_vals()
        return vals

    def get_thickness(self):
        return self.marching_tets.interp_coef()

    def init_coef(self, target):
        optimizer = torch.optim.Adam(self.marching_tets.interp_coef.parameters(), lr=1e-1)
        for _ in range(3000):
            coef = self.marching_tets.interp_coef()
            loss = (coef - target) ** 2
            optimizer.zero_grad()
            loss.backward()
            optimizer.step()
        print(f"coef init to {self.marching_tets.interp_coef().item()}")
