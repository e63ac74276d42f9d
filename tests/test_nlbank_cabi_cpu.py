"""The tension-modulated bank's entry points resolve on a CPU-only box, are declared in the header, bound in _hip and built
by the Makefile, refuse bad arguments before any device work, in the documented order, and ask for a workspace that does not
grow with the oversampling factor beyond one segment a clip."""
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _cabi import assert_refused, hip_built as _hip_built, refusal_calls, symbols_declared  # noqa: E402

NAMES = ("ds_nlbank_workspace_bytes", "ds_nlbank_fwd", "ds_nlbank_bwd")


def test_nlbank_symbols():
    header, src = symbols_declared(NAMES, "nlbank.hip")
    _hip = _hip_built()
    assert re.search(r"#define DS_NLBANK_MAX_MODES 512\b", header)
    assert re.search(r"#define DS_NLBANK_MAX_TERMS 4\b", header)
    assert re.search(r"#define DS_NLBANK_MAX_OVERSAMPLE 64\b", header)
    assert re.search(r"#define DS_NLBANK_MAX_CLIPS 65535\b", header)
    assert re.search(r"#define DS_NLBANK_MAX_SUBSTEPS 16777216\b", header)
    assert _hip.lib().ds_abi_version() == 45 == _hip.ABI_VERSION  # three added symbols, no bump
    assert "__shared__" not in src and "__syncthreads" not in src
    assert "atomic" not in src.replace("no atomics", "")
    assert "#pragma clang fp contract(off)" in src
    from diffsound_amd.ddsp import nonlinear

    assert (nonlinear.MAX_MODES, nonlinear.MAX_TERMS, nonlinear.MAX_OVERSAMPLE, nonlinear.MAX_CLIPS, nonlinear.MAX_SUBSTEPS) == \
        (512, 4, 64, 65535, 1 << 24)


OK = 1 << 20  # never dereferenced: the checks come first
GOOD = dict(gy=OK, d=OK, w=OK, gain=OK, amp=OK, f=OK, C=OK, gamma=OK, A=2, m=3, K=2, F=7, S=5, R=4, sr=44100.0, work=OK,
            bytes=1 << 16, y=OK, gd=OK, gw=OK, ggain=OK, gamp=OK, gf=OK, gC=OK, ggamma=OK)
FWD = ("d", "w", "gain", "amp", "f", "C", "gamma", "A", "m", "K", "F", "S", "R", "sr", "y")
BWD = ("gy", "d", "w", "gain", "amp", "f", "C", "gamma", "A", "m", "K", "F", "S", "R", "sr", "work", "bytes", "gd", "gw", "ggain",
       "gamp", "gf", "gC", "ggamma")
NEED = 16 * (2 * 5 * 3 + 2 * 4 * 3 + 2 * 3) + 8 * 2 * 2 * 3  # 16 (A S m + A R m + A m) + 8 A K m
BAD = [(dict(d=None), "null pointer"), (dict(w=None), "null pointer"), (dict(gain=None), "null pointer"),
       (dict(amp=None), "null pointer"), (dict(f=None), "null pointer"), (dict(C=None), "null pointer"),
       (dict(gamma=None), "null pointer"),
       (dict(A=0), "A = 0 outside 1..65535"), (dict(A=-1), "outside 1..65535"), (dict(A=65536), "outside 1..65535"),
       (dict(m=0), "m = 0 outside 1..512"), (dict(m=513), "m = 513 outside 1..512"),
       (dict(K=0), "K = 0 outside 1..4"), (dict(K=5), "K = 5 outside 1..4"),
       (dict(R=0), "R = 0 outside 1..64"), (dict(R=65), "R = 65 outside 1..64"),
       (dict(F=0), "F = 0 below 1"), (dict(F=-3), "below 1"), (dict(S=0), "S = 0 below 1"), (dict(S=-3), "below 1"),
       (dict(S=(1 << 24) // 4 + 1), "substeps above 16777216"), (dict(S=1 << 30, R=64), "substeps above 16777216"),
       (dict(sr=0.0), "not positive"), (dict(sr=-1.0), "not positive"), (dict(sr=float("nan")), "not positive"),
       (dict(d=OK + 4), "misaligned operand"), (dict(amp=OK + 4), "misaligned operand"), (dict(gamma=OK + 2), "misaligned operand"),
       (dict(C=OK + 4), "misaligned operand"), (dict(f=OK + 4), "misaligned operand")]
BAD_FWD = [(dict(y=None), "null pointer"), (dict(y=OK + 2), "misaligned operand")]
BAD_BWD = [(dict(gy=None), "null pointer"), (dict(work=None), "null pointer"),
           (dict(gd=None), "gd and gw go together"), (dict(gw=None), "gd and gw go together"),
           (dict(bytes=NEED - 1), "bytes, %d needed" % NEED), (dict(bytes=0), "needed"), (dict(work=OK + 8), "work not 16-byte aligned"),
           (dict(gy=OK + 2), "misaligned operand"), (dict(ggain=OK + 4), "misaligned operand"), (dict(gamp=OK + 4), "misaligned operand"),
           (dict(gf=OK + 4), "misaligned operand"), (dict(gC=OK + 4), "misaligned operand"), (dict(ggamma=OK + 4), "misaligned operand")]
# two things wrong: the one that is listed first is the one that is named
ORDER = [(dict(d=None, A=0), "null pointer"), (dict(A=0, m=0), "A = 0 outside"), (dict(m=0, K=0), "m = 0 outside"),
         (dict(K=0, R=0), "K = 0 outside"), (dict(R=0, F=0), "R = 0 outside"), (dict(F=0, S=0), "F = 0 below 1"),
         (dict(S=0, sr=0.0), "S = 0 below 1"), (dict(S=1 << 30, sr=0.0), "substeps above")]
ORDER_BWD = [(dict(sr=0.0, gd=None), "not positive"), (dict(gd=None, bytes=0), "gd and gw go together"),
             (dict(bytes=0, work=OK + 8), "needed"), (dict(work=OK + 8, d=OK + 4), "work not 16-byte aligned")]
CALLS, IDS = refusal_calls(("ds_nlbank_fwd", FWD), ("ds_nlbank_bwd", BWD), BAD, BAD_FWD, BAD_BWD, ORDER, ORDER_BWD, id_from=10,
                           id_sep="-")


@pytest.mark.parametrize("fn,order,change,text", CALLS, ids=IDS)
def test_nlbank_arguments_are_checked_first(fn, order, change, text):
    """Every host-side refusal: DS_ERR_ARG and a message that names the entry point and the reason, in front of any launch."""
    assert_refused(fn, order, GOOD, change, text, status=1)


@pytest.mark.parametrize("fn,order", [("ds_nlbank_fwd", FWD), ("ds_nlbank_bwd", BWD)], ids=["fwd", "bwd"])
def test_limits_at_their_edges_pass_the_shape_checks(fn, order):
    """Each limit AT its edge is no refusal reason: the call goes on to a later check, here a misaligned d (the last one)."""
    for edge in (dict(A=65535), dict(m=512), dict(K=4), dict(R=64), dict(S=(1 << 24) // 4), dict(S=1 << 18, R=64), dict(A=1, m=1, K=1,
                 R=1, F=1, S=1)):
        assert_refused(fn, order, GOOD, dict(edge, d=OK + 4, bytes=1 << 62), "misaligned operand", status=1)


def test_a_null_gradient_group_is_no_refusal_reason():
    """gd with gw, ggain, gamp, gf, gC, ggamma: each group may be NULL; with all of them NULL the call is refused only further
    on, here for its workspace."""
    change = dict(gd=None, gw=None, ggain=None, gamp=None, gf=None, gC=None, ggamma=None, bytes=0)
    assert_refused("ds_nlbank_bwd", BWD, GOOD, change, "needed", status=1)
    for one in ("ggain", "gamp", "gf", "gC", "ggamma"):
        assert_refused("ds_nlbank_bwd", BWD, GOOD, {one: None, "bytes": 0}, "needed", status=1)


def test_nlbank_workspace_query_needs_no_device():
    q = _hip_built().lib().ds_nlbank_workspace_bytes
    closed = lambda A, m, K, S, R: 16 * (A * S * m + A * R * m + A * m) + 8 * A * K * m  # noqa: E731
    assert q(2, 3, 2, 5, 4) == NEED == closed(2, 3, 2, 5, 4)
    assert q(64, 64, 1, 512, 8) == closed(64, 64, 1, 512, 8)
    assert q(65535, 512, 4, 1 << 24, 1) == closed(65535, 512, 4, 1 << 24, 1) > 1 << 32
    # R enters through the one segment a clip and nowhere else, K through the gC partials
    for A, m, S in ((1, 1, 1), (8, 64, 32000), (3, 130, 33)):
        for K in (1, 4):
            assert q(A, m, K, S, 1) == closed(A, m, K, S, 1)
            for R in (2, 8, 64):
                assert q(A, m, K, S, R) - q(A, m, K, S, 1) == 16 * A * (R - 1) * m
        assert q(A, m, 4, S, 8) - q(A, m, 1, S, 8) == 8 * A * 3 * m
    # the record that is not kept: 8 x 32000 x 8 x 64 substep states are 2.1 GB, the checkpoints 0.26 GB
    assert q(8, 64, 4, 32000, 8) < 16 * 8 * 32000 * 8 * 64 // 7
    for a in [(0, 3, 2, 5, 4), (65536, 3, 2, 5, 4), (2, 0, 2, 5, 4), (2, 513, 2, 5, 4), (2, 3, 0, 5, 4), (2, 3, 5, 5, 4),
              (2, 3, 2, 0, 4), (2, 3, 2, 5, 0), (2, 3, 2, 5, 65), (2, 3, 2, (1 << 24) // 4 + 1, 4), (2, 3, 2, 1 << 30, 64),
              (-1, 3, 2, 5, 4)]:
        assert q(*a) == 0
    for a in [(65535, 3, 2, 5, 4), (2, 512, 2, 5, 4), (2, 3, 4, 5, 4), (2, 3, 2, 5, 64), (2, 3, 2, (1 << 24) // 4, 4)]:
        assert q(*a) == closed(*a)


def test_python_layer_refuses_before_device_work():
    """The checks of ``nonlinear_bank`` need no device: ValueError on a CPU-only box, and RuntimeError for CPU tensors that
    pass them."""
    import torch

    from diffsound_amd.ddsp import TensionModulatedBank, modal_stretch, nonlinear_bank
    from src.ddsp.nonlinear import TensionModulatedBank as alias

    assert alias is TensionModulatedBank and callable(modal_stretch)
    f64 = lambda *v: torch.tensor(v, dtype=torch.float64)  # noqa: E731
    ones = lambda *s: torch.ones(*s, dtype=torch.float64)  # noqa: E731
    good = dict(d=f64(3.0, 4.0), w=f64(3e3, 9e3), gain=ones(2, 2), amp=ones(2, 2), force=ones(2, 8), stretch=ones(3, 2),
                coupling=ones(2, 3), sample_num=16, sr=44100.0)
    nan = float("nan")
    bad = [(dict(w=f64(3e3, 0.0)), "w must be positive"), (dict(w=f64(-3e3, 9e3)), "w must be positive"),
           (dict(stretch=-ones(3, 2)), "stretch must not be negative"), (dict(coupling=-ones(2, 3)), "coupling must not be negative"),
           (dict(d=f64(3.0, nan)), "d is not finite"), (dict(force=ones(2, 8) * float("inf")), "force is not finite"),
           (dict(gain=ones(2, 2) * nan), "gain is not finite"), (dict(amp=ones(2, 2) * nan), "amp is not finite"),
           (dict(stretch=ones(3, 2) * nan), "stretch is not finite"), (dict(coupling=ones(2, 3) * nan), "coupling is not finite"),
           (dict(w=f64(3e3, 9e3, 1e4)), r"d and w must be \(m,\)"), (dict(gain=ones(2, 3)), r"gain must be \(A, 2\)"),
           (dict(gain=ones(2)), r"gain must be \(A, 2\)"), (dict(amp=ones(3, 2)), r"amp must be \(2, 2\)"),
           (dict(force=ones(3, 8)), r"force must be \(2, F\)"), (dict(force=ones(2, 0)), r"force must be \(2, F\)"),
           (dict(stretch=ones(3, 3)), r"stretch must be \(K, 2\)"), (dict(stretch=ones(2)), r"stretch must be \(K, 2\)"),
           (dict(coupling=ones(2, 2)), r"coupling must be \(2, 3\)"), (dict(coupling=ones(3)), r"coupling must be \(2, 3\)"),
           (dict(d=ones(513), w=ones(513), gain=ones(2, 513), amp=ones(2, 513), stretch=ones(3, 513)), "outside 1..512"),
           (dict(stretch=ones(5, 2), coupling=ones(2, 5)), "K = 5 outside 1..4"),
           (dict(oversample=0), "oversample = 0"), (dict(oversample=65), "oversample = 65"),
           (dict(sample_num=(1 << 24) // 8 + 1), "substeps"), (dict(sample_num=0), "sample_num = 0 below 1"),
           (dict(sr=0.0), "sr"), (dict(sr=nan), "sr"), (dict(d=[3.0, 4.0]), "d must be a floating-point tensor")]
    for change, text in bad:
        with pytest.raises(ValueError, match=text):
            nonlinear_bank(**dict(good, **change))
    with pytest.raises(RuntimeError, match="HIP device"):
        nonlinear_bank(**good)
    bank = TensionModulatedBank(2, ones(3, 2), coupling=[1.0, 2.0, 4.0], oversample=4)
    assert bank.log_coupling.dtype == bank.stretch.dtype == torch.float64 and bank.log_coupling.requires_grad
    assert bank.log_coupling.shape == (2, 3) and bank.stretch.shape == (3, 2) and "stretch" in dict(bank.named_buffers())
    assert torch.equal(bank.log_coupling.detach().exp().round(), f64(1.0, 2.0, 4.0).expand(2, 3))
    assert not TensionModulatedBank(2, ones(2), train_coupling=False).log_coupling.requires_grad
    assert TensionModulatedBank(2, ones(2)).stretch.shape == (1, 2)
    with pytest.raises(RuntimeError, match="HIP device"):
        bank(good["d"], good["w"], good["gain"], good["amp"], good["force"], 16, 44100.0)
    for kw, text in ((dict(coupling=0.0), "coupling must be positive"), (dict(coupling=[1.0, 2.0]), "coupling must be a number"),
                     (dict(stretch=-ones(3, 2)), "stretch must be finite"), (dict(stretch=ones(5, 2)), "stretch must be"),
                     (dict(oversample=65), "oversample"), (dict(audio_num=0), "audio_num")):
        args = dict(dict(audio_num=2, stretch=ones(3, 2)), **kw)
        with pytest.raises(ValueError, match=text):
            TensionModulatedBank(**args)
