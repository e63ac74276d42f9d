"""The friction entry points resolve on a CPU-only box, are declared in the header, bound in _hip and built by the
Makefile, refuse bad arguments before any device work, in the documented order, and ask for a workspace that does not grow
with the oversampling factor beyond one segment a clip."""
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _cabi import assert_refused, hip_built as _hip_built, refusal_calls, symbols_declared  # noqa: E402

NAMES = ("ds_friction_workspace_bytes", "ds_friction_fwd", "ds_friction_bwd")


def test_friction_symbols():
    header, src = symbols_declared(NAMES, "friction.hip")
    _hip = _hip_built()
    assert re.search(r"#define DS_FRICTION_MAX_MODES 512\b", header)
    assert re.search(r"#define DS_FRICTION_MAX_OVERSAMPLE 64\b", header)
    assert re.search(r"#define DS_FRICTION_MAX_CLIPS 65535\b", header)
    assert _hip.lib().ds_abi_version() == 45 == _hip.ABI_VERSION  # three added symbols, no bump
    assert "__shared__" not in src and "__syncthreads" not in src
    assert "atomic" not in src.replace("no atomics", "")
    assert "#pragma clang fp contract(off)" in src


OK = 1 << 20  # never dereferenced: the checks come first
GOOD = dict(gforce=OK, d=OK, w=OK, gain=OK, vb=OK, N=OK, vs=OK, A=2, m=3, F=5, R=4, sr=44100.0, work=OK, bytes=1 << 16, force=OK,
            gd=OK, gw=OK, ggain=OK, gvb=OK, gN=OK, gvs=OK)
FWD = ("d", "w", "gain", "vb", "N", "vs", "A", "m", "F", "R", "sr", "force")
BWD = ("gforce", "d", "w", "gain", "vb", "N", "vs", "A", "m", "F", "R", "sr", "work", "bytes", "gd", "gw", "ggain", "gvb", "gN", "gvs")
NEED = 16 * (2 * 5 * 3 + 2 * 4 * 3 + 2 * 3)  # 16 (A F m + A R m + A m)
BAD = [(dict(d=None), "null pointer"), (dict(w=None), "null pointer"), (dict(gain=None), "null pointer"),
       (dict(vb=None), "null pointer"), (dict(N=None), "null pointer"), (dict(vs=None), "null pointer"),
       (dict(A=0), "A = 0 outside 1..65535"), (dict(A=-1), "outside 1..65535"), (dict(A=65536), "outside 1..65535"),
       (dict(m=0), "m = 0 outside 1..512"), (dict(m=513), "m = 513 outside 1..512"),
       (dict(R=0), "R = 0 outside 1..64"), (dict(R=65), "R = 65 outside 1..64"),
       (dict(F=0), "F = 0 below 1"), (dict(F=-3), "below 1"),
       (dict(F=(1 << 24) // 4 + 1), "substeps above 16777216"), (dict(F=1 << 30, R=64), "substeps above 16777216"),
       (dict(sr=0.0), "not positive"), (dict(sr=-1.0), "not positive"), (dict(sr=float("nan")), "not positive"),
       (dict(d=OK + 4), "misaligned operand"), (dict(gain=OK + 4), "misaligned operand"), (dict(vs=OK + 2), "misaligned operand")]
BAD_FWD = [(dict(force=None), "null pointer"), (dict(force=OK + 2), "misaligned operand")]
BAD_BWD = [(dict(gforce=None), "null pointer"), (dict(work=None), "null pointer"),
           (dict(gd=None), "gd and gw go together"), (dict(gw=None), "gd and gw go together"),
           (dict(gvb=None), "gvb and gN go together"), (dict(gN=None), "gvb and gN go together"),
           (dict(bytes=NEED - 1), "bytes, %d needed" % NEED), (dict(bytes=0), "needed"), (dict(work=OK + 8), "work not 16-byte aligned"),
           (dict(gforce=OK + 2), "misaligned operand"), (dict(ggain=OK + 4), "misaligned operand"), (dict(gvs=OK + 4), "misaligned operand")]
# two things wrong: the one that is listed first is the one that is named
ORDER = [(dict(d=None, A=0), "null pointer"), (dict(A=0, m=0), "A = 0 outside"), (dict(m=0, R=0), "m = 0 outside"),
         (dict(R=0, F=0), "R = 0 outside"), (dict(F=0, sr=0.0), "F = 0 below 1"), (dict(F=1 << 30, sr=0.0), "substeps above")]
ORDER_BWD = [(dict(sr=0.0, gd=None), "not positive"), (dict(gd=None, gvb=None), "gd and gw go together"),
             (dict(gvb=None, bytes=0), "gvb and gN go together"), (dict(bytes=0, work=OK + 8), "needed"),
             (dict(work=OK + 8, d=OK + 4), "work not 16-byte aligned")]
CALLS, IDS = refusal_calls(("ds_friction_fwd", FWD), ("ds_friction_bwd", BWD), BAD, BAD_FWD, BAD_BWD, ORDER, ORDER_BWD, id_from=12,
                           id_sep="-")


@pytest.mark.parametrize("fn,order,change,text", CALLS, ids=IDS)
def test_friction_arguments_are_checked_first(fn, order, change, text):
    """Every host-side refusal: DS_ERR_ARG and a message that names the entry point and the reason, in front of any launch."""
    assert_refused(fn, order, GOOD, change, text, status=1)


def test_a_null_gradient_group_is_no_refusal_reason():
    """gd with gw, ggain, gvb with gN, gvs: each group may be NULL; with all of them NULL the call is refused only further on,
    here for its workspace."""
    change = dict(gd=None, gw=None, ggain=None, gvb=None, gN=None, gvs=None, bytes=0)
    assert_refused("ds_friction_bwd", BWD, GOOD, change, "needed", status=1)


def test_friction_workspace_query_needs_no_device():
    q = _hip_built().lib().ds_friction_workspace_bytes
    assert q(2, 3, 5, 4) == NEED
    assert q(64, 64, 512, 8) == 16 * (64 * 512 * 64 + 64 * 8 * 64 + 64 * 64)
    assert q(65535, 512, 1 << 24, 1) == 16 * (65535 * (1 << 24) * 512 + 65535 * 512 + 65535 * 512)  # beyond 2^32
    # R enters through the one segment a clip and nowhere else
    for A, m, F in ((1, 1, 1), (8, 64, 32000), (3, 130, 33)):
        assert q(A, m, F, 1) == 16 * (A * F * m + A * m + A * m)
        for R in (2, 8, 64):
            assert q(A, m, F, R) - q(A, m, F, 1) == 16 * A * (R - 1) * m
            assert q(A, m, F, R) <= 16 * (A * F * m + A * R * m + A * m)
    # the record that is not kept: 8 x 32000 x 8 x 64 substep states are 2.1 GB, the checkpoints 0.26 GB
    assert q(8, 64, 32000, 8) < 16 * 8 * 32000 * 8 * 64 // 7
    for a in [(0, 3, 5, 4), (65536, 3, 5, 4), (2, 0, 5, 4), (2, 513, 5, 4), (2, 3, 0, 4), (2, 3, 5, 0), (2, 3, 5, 65),
              (2, 3, (1 << 24) // 4 + 1, 4), (2, 3, 1 << 30, 64), (-1, 3, 5, 4)]:
        assert q(*a) == 0


def test_python_layer_refuses_before_device_work():
    """The checks of ``friction_force`` need no device: ValueError on a CPU-only box, and RuntimeError for CPU tensors that
    pass them."""
    import torch

    from diffsound_amd.ddsp import Bow, friction_force
    from src.ddsp.friction import Bow as alias

    assert alias is Bow
    f64 = lambda *v: torch.tensor(v, dtype=torch.float64)  # noqa: E731
    ones = lambda *s: torch.ones(*s, dtype=torch.float64)  # noqa: E731
    good = dict(d=f64(3.0, 4.0), w=f64(3e3, 9e3), gain=ones(2, 2), bow_velocity=0.2 * ones(2, 8), normal_force=ones(2, 8),
                stribeck_velocity=f64(0.1, 0.1), sr=44100.0)
    nan = float("nan")
    bad = [(dict(w=f64(3e3, 0.0)), "w must be positive"), (dict(w=f64(-3e3, 9e3)), "w must be positive"),
           (dict(d=f64(3.0, 0.0)), "d must be positive"), (dict(normal_force=-ones(2, 8)), "normal_force must not be negative"),
           (dict(stribeck_velocity=f64(0.1, 0.0)), "stribeck_velocity must be positive"),
           (dict(d=f64(3.0, nan)), "d is not finite"), (dict(bow_velocity=ones(2, 8) * float("inf")), "bow_velocity is not finite"),
           (dict(normal_force=ones(2, 8) * nan), "normal_force is not finite"), (dict(gain=ones(2, 2) * nan), "gain is not finite"),
           (dict(stribeck_velocity=f64(0.1, nan)), "stribeck_velocity is not finite"),
           (dict(w=f64(3e3, 9e3, 1e4)), r"d and w must be \(m,\)"), (dict(gain=ones(2, 3)), r"gain must be \(A, 2\)"),
           (dict(gain=ones(2)), r"gain must be \(A, 2\)"), (dict(bow_velocity=ones(3, 8)), r"bow_velocity must be \(2, F\)"),
           (dict(bow_velocity=ones(2, 0), normal_force=ones(2, 0)), r"bow_velocity must be \(2, F\)"),
           (dict(normal_force=ones(2, 7)), r"normal_force must be \(2, 8\)"), (dict(stribeck_velocity=f64(0.1)), r"stribeck_velocity must be \(2,\)"),
           (dict(d=ones(513), w=ones(513), gain=ones(2, 513)), "outside 1..512"),
           (dict(oversample=0), "oversample = 0"), (dict(oversample=65), "oversample = 65"), (dict(sr=0.0), "sr"),
           (dict(d=[3.0, 4.0]), "d must be a floating-point tensor")]
    for change, text in bad:
        with pytest.raises(ValueError, match=text):
            friction_force(**dict(good, **change))
    with pytest.raises(RuntimeError, match="HIP device"):
        friction_force(**good)
    bow = Bow(2, 8, 44100.0, 0.2, 1.0, attack=2 / 44100.0, release=2 / 44100.0)
    assert bow.velocity.dtype == bow.log_pressure.dtype == bow.log_stribeck.dtype == torch.float64
    assert bow.velocity.shape == bow.log_pressure.shape == bow.log_stribeck.shape == (2,)
    with pytest.raises(RuntimeError, match="HIP device"):
        bow(good["d"], good["w"], good["gain"])
    with pytest.raises(ValueError, match="must be positive"):
        Bow(2, 8, 44100.0, 0.2, 0.0)
    with pytest.raises(ValueError, match="must be positive"):
        Bow(2, 8, 44100.0, 0.2, 1.0, stribeck_velocity=-0.1)


def test_bow_gesture_is_the_envelope_times_the_parameters():
    import numpy as np
    import torch

    import _friction_ref as Fr
    from diffsound_amd.ddsp import Bow

    bow = Bow(2, 64, Fr.SR, [0.2, -0.1], [3.0, 5.0], attack=8 / Fr.SR, release=16 / Fr.SR, train_pressure=False)
    assert bow.velocity.requires_grad and not bow.log_pressure.requires_grad and bow.log_stribeck.requires_grad
    vb, N = bow.gesture()
    env = Fr.envelope(64, Fr.SR, 8 / Fr.SR, 16 / Fr.SR)
    assert vb.shape == N.shape == (2, 64) and vb.dtype == N.dtype == torch.float64
    assert np.allclose(vb.detach().numpy(), np.array([[0.2], [-0.1]]) * env, rtol=0, atol=1e-15)
    assert np.allclose(N.detach().numpy(), np.array([[3.0], [5.0]]) * env, rtol=1e-15, atol=1e-15)
    assert float(N.min()) == 0.0  # the envelope starts and ends at exactly 0: no negative normal force from rounding
