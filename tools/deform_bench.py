"""Performance and memory record of the Deform operators (csrc/deform.hip through diffsound_amd/diffelastic/deform.py).

Two meshes: the benchmark's (a 26^3 Kuhn box lifted to order 2: 105 456 elements, 64 Gauss points each) and an order-1
mesh of the size the shape loops solve (a 32^3 Kuhn box: 196 608 elements, 27 Gauss points each); 1 and 8 columns.
Per case and per operation - ``gradient`` (gradient_batch), ``force`` (stress_to_force_batch), ``gradient_backward``
(the force without the integration weights) and ``force_backward`` (the gradient times them), the backward passes
timed as autograd runs them -

* ``native_ms``: median over ``--reps`` calls between device events, after a warm-up; ``native_peak_bytes``: the
  largest allocation of one call above what was resident before it (inputs excluded);
* ``torch_ms`` / ``torch_peak_bytes``: the same operation in the torch formulation of the reference on the same
  device - the materialised B (T*G, N, 3), the materialised index map and ``index_add_`` - with the tables built
  beforehand and counted under ``torch_resident_bytes``; it runs a column at a time (see ``TorchDeform``), so its
  time is the sum over the columns and its peak is one column's temporaries plus the result;
* ``max_rel_diff``: the largest difference of the two results over the largest magnitude.

``triad_bytes_per_s``: csrc/stream.hip's triad (3 x 4 bytes per element) on 2^28 floats in the same run, and per case
``gradient_write_fraction_of_triad`` = the bytes of F over ``native_ms`` of the gradient, divided by it.
Writes one JSON document to ``--out`` (default profiles/deform_bench.json; ``-`` for stdout)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps):
    """(median ms between device events, peak bytes of one call above the resident set)."""
    fn()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), int(peak)


class TorchDeform:
    """The reference's formulation (deform.py:35-68, 70-87, 113-125, 149-166) as torch ops on the device."""

    def __init__(self, deform):
        self.d = deform
        self.B = deform.shape_func_deriv
        self.w = deform.integration_weights
        self.index = deform.stress_index
        self.nv = deform.tetmesh.vertices.shape[0]

    def resident_bytes(self):
        return sum(t.numel() * t.element_size() for t in (self.B, self.w, self.index))

    # A column at a time: at 8 columns of the ord-2 mesh the gathered nodal values and the broadcast B are 6.5 GB each,
    # and the batched matmul over operands beyond 4 GB faulted on the device (hipErrorIllegalAddress) where one column
    # (0.8 GB) runs.  The columns are independent, so the time of a call is the sum over its columns.
    def gradient(self, u, weighted=False):
        return torch.cat([self._gradient(u[b:b + 1], weighted) for b in range(u.shape[0])])

    def force(self, P, weighted=True):
        return torch.cat([self._force(P[b:b + 1], weighted) for b in range(P.shape[0])])

    def _gradient(self, u, weighted):
        d = self.d
        ue = u[:, d.tetmesh.tets].transpose(2, 3)
        ue = ue.unsqueeze(2).repeat(1, 1, d.num_guass_points, 1, 1).reshape(-1, d.num_tets * d.num_guass_points, 3,
                                                                           d.num_nodes_per_tet)
        F = ue @ self.B
        return F * self.w if weighted else F

    def _force(self, P, weighted):
        force = P @ self.B.transpose(1, 2)
        if weighted:
            force = force * self.w
        force = force.transpose(2, 3).reshape(force.shape[0], -1)
        out = torch.zeros((force.shape[0], 3 * self.nv), dtype=force.dtype, device=force.device)
        return out.index_add_(1, self.index, force)


def triad(n=1 << 28, reps=20):
    from diffsound_amd import _hip

    a, b, c = (torch.rand(n, device="cuda") for _ in range(3))
    run = lambda: _hip.check(_hip.lib().ds_stream_triad(a.data_ptr(), b.data_ptr(), c.data_ptr(), n, 0.5, _hip.stream_ptr()),
                             "ds_stream_triad")
    ms, _ = timed(run, reps)
    return 12.0 * n / (ms * 1e-3)


def relmax(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deform_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("deform_bench: no HIP device (a timing taken elsewhere says nothing)")
    from diffsound_amd import meshgen
    from diffsound_amd.diffelastic.deform import Deform
    from diffsound_amd.diffelastic.mesh import TetMesh

    dev = torch.device("cuda:0")
    rec = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "triad_bytes_per_s": triad(), "cases": []}
    for name, cells, order in (("bench_ord2_105456", 26, 2), ("shape_ord1_196608", 32, 1)):
        v, t = meshgen.kuhn_box(cells)
        mesh = TetMesh(torch.from_numpy(v).float().to(dev), torch.from_numpy(t).long().to(dev)).to_high_order(order)
        deform = Deform(mesh)
        nv, tg = mesh.vertices.shape[0], deform.num_tets * deform.num_guass_points
        ref = TorchDeform(deform)
        for batch in (1, 8):
            gen = torch.Generator(device=dev).manual_seed(batch)
            u = torch.randn((batch, nv, 3), device=dev, generator=gen)
            P = torch.randn((batch, tg, 3, 3), device=dev, generator=gen)
            ops = {
                "gradient": (lambda: deform.gradient_batch(u), lambda: ref.gradient(u)),
                "force": (lambda: deform.stress_to_force_batch(P), lambda: ref.force(P)),
                "gradient_backward": (lambda: deform.stress_to_force_batch(P, weighted=False), lambda: ref.force(P, False)),
                "force_backward": (lambda: deform.gradient_batch(u, weighted=True), lambda: ref.gradient(u, True)),
            }
            case = {"name": name, "order": order, "elements": deform.num_tets, "nodes": nv, "gauss_points": tg,
                    "columns": batch, "F_bytes": batch * tg * 36, "torch_resident_bytes": ref.resident_bytes(), "ops": {}}
            for op, (native, torch_form) in ops.items():
                nms, npeak = timed(native, args.reps)
                tms, tpeak = timed(torch_form, max(3, args.reps // 4))
                case["ops"][op] = {"native_ms": nms, "native_peak_bytes": npeak, "torch_ms": tms, "torch_peak_bytes": tpeak,
                                   "torch_over_native": tms / nms, "max_rel_diff": relmax(native(), torch_form())}
            # autograd end to end, as stiff_func's backward runs it
            ug = u.clone().requires_grad_(True)
            case["autograd_gradient_backward_ms"] = timed(
                lambda: torch.autograd.grad((deform.gradient_batch(ug) * P).sum(), ug), max(3, args.reps // 4))[0]
            wr = case["F_bytes"] / (case["ops"]["gradient"]["native_ms"] * 1e-3)
            case["gradient_write_bytes_per_s"] = wr
            case["gradient_write_fraction_of_triad"] = wr / rec["triad_bytes_per_s"]
            rec["cases"].append(case)
            print(json.dumps(case), file=sys.stderr, flush=True)
            del u, P, ug
        del ref, deform
        torch.cuda.empty_cache()
    text = json.dumps(rec, indent=1)
    if args.out != "-":
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    else:
        print(text)


if __name__ == "__main__":
    main()
