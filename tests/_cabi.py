"""What the test_*_cabi_cpu.py files share (not a test module): the built library, the check that a family of entry points
is bound, exported, declared and built, and the table-driven test of their host-side refusals.  A file keeps its own tables
(GOOD, BAD, ORDER, ...) and its own parametrised test; the bodies are here."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "diffsound_amd", "csrc")


def hip_built():
    """diffsound_amd._hip with its library in place (built first where it is missing)."""
    from diffsound_amd import _hip

    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return _hip


def symbols_declared(names, source_file):
    """Every name is bound in _hip, resolves on the library and is declared in the header, and the Makefile builds
    ``source_file`` of csrc/.  Returns (header text, source text) for the caller's own assertions."""
    _hip = hip_built()
    lib = _hip.lib()
    header = open(os.path.join(ROOT, "include", "diffsound_hip.h")).read()
    for name in names:
        assert name in _hip.EXPORTED_SYMBOLS and name in _hip._SIGNATURES and hasattr(lib, name), name
        assert re.search(r"\b%s\s*\(" % name, header), name
    assert re.search(r"\b%s\b" % re.escape(source_file), open(os.path.join(CSRC, "Makefile")).read())
    return header, open(os.path.join(CSRC, source_file)).read()


def refusal_calls(fwd, bwd, bad, bad_fwd, bad_bwd, order=(), order_bwd=(), id_from=3, id_sep=","):
    """(calls, ids) of a refusal table.  ``fwd`` / ``bwd``: (entry point, the names of its arguments in order); ``bad`` goes to
    both, ``bad_fwd`` / ``bad_bwd`` to one; ``order`` / ``order_bwd`` likewise for the cases with two things wrong, which
    come last.  A call is (fn, argument names, change, text); its id is the entry point from character ``id_from`` on and
    the changed arguments joined by ``id_sep``."""
    calls = ([(fwd[0], fwd[1], c, t) for c, t in list(bad) + list(bad_fwd)] + [(bwd[0], bwd[1], c, t) for c, t in list(bad) + list(bad_bwd)] +
             [(fn, names, c, t) for fn, names in (fwd, bwd) for c, t in order] + [(bwd[0], bwd[1], c, t) for c, t in order_bwd])
    return calls, [f"{fn[id_from:]}-" + id_sep.join(f"{k}={v}" for k, v in c.items()) for fn, _, c, _ in calls]


def assert_refused(fn, order, good, change, text, status=None):
    """``fn`` with ``good`` changed by ``change`` (and a null stream) is refused on the host - a non-zero status, or exactly
    ``status`` - with a message that names the entry point and holds ``text``.  The pointers of ``good`` are fakes that a
    launch would fault on; the call needs no device."""
    lib = hip_built().lib()
    got = getattr(lib, fn)(*[dict(good, **change)[k] for k in order], None)
    assert got != 0 if status is None else got == status, got
    msg = lib.ds_last_error().decode()
    assert fn in msg and text in msg, msg
