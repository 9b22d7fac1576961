"""Textual check of the fit-ensemble wrappers of julia/KANODEHip.jl against include/kanode.h (Julia is not in this
image, so the shim is not executed), in the manner of tests/test_julia_ensemble_solve.py: the new entry has the
argument list of kanode_train_ensemble_tsit5, so the wrapper goes through train_ensemble_call (one ccall tuple, one
per-replica length check) and asks the coverage first."""
import re

from test_julia_shim import HDR, JL, _strip


def _functions(src):
    """name -> bodies of the top-level `function name(...) ... end` blocks, names ending in `!` included."""
    out = {}
    for m in re.finditer(r"^function ([\w.]+!?)\(.*?^end\b", src, flags=re.S | re.M):
        out.setdefault(m.group(1), []).append(m.group(0))
    return out


def header_args(name):
    decl = re.search(r"\b" + name + r"\s*\((.*?)\)\s*;", HDR, flags=re.S).group(1)
    return [re.sub(r"\s+", " ", a.strip()) for a in decl.split(",")]


def test_header_entry_has_the_ensemble_argument_list():
    fit = header_args("kanode_fit_ensemble_tsit5")
    twin = header_args("kanode_train_ensemble_tsit5")
    assert fit == twin and len(fit) == 32
    assert header_args("kanode_fit_ensemble_supported") == ["const kanode_handle* h", "int64_t batch"]


def test_ccall_goes_through_the_shared_ensemble_call():
    fns = _functions(_strip(JL))
    body = fns["fit_ensemble_tsit5!"][0]
    assert "train_ensemble_call(:kanode_fit_ensemble_tsit5, h, R, p, m, v, u0, B," in body
    assert "ccall" not in body                                   # (the one ccall tuple is train_ensemble_call's)
    shared = fns["train_ensemble_call"][0]
    types = re.search(r"ccall\(sym\(name\), Cint,\s*\((.*?)\),\s*\n\s*h\.ptr", shared, flags=re.S).group(1)
    assert len([t for t in re.sub(r"\s+", " ", types).split(", ") if t]) == 32
    # the same parameter-length check as train_ensemble_tsit5!: one entry of η, l1 and βp per replica
    assert "length(ηv) == R && length(βv) == 2R && (l1 === nothing || length(l1v) == R)" in shared
    assert "DimensionMismatch" in shared and shared.index("DimensionMismatch") < shared.index("ccall")


def test_wrapper_asks_the_coverage_before_the_call():
    body = _functions(_strip(JL))["fit_ensemble_tsit5!"][0]
    call = body.index("train_ensemble_call(")
    for must in ("fit_ensemble_supported(h, B)", "ArgumentError", "l1 isa Real ? fill(Float64(l1), R) : l1"):
        assert must in body and body.index(must) < call, must
    assert re.search(r"fit_ensemble_supported\(h::Handle, B::Integer\) =\s*\n\s*ccall\(sym\(:kanode_fit_ensemble_supported\), "
                     r"Int32, \(Ptr\{Cvoid\}, Int64\), h\.ptr, B\) == 1", JL)
    # beside train_ensemble_tsit5!, and after the shared call it uses
    assert JL.index("function train_ensemble_call(") < JL.index("function train_ensemble_tsit5!(") \
        < JL.index("function fit_ensemble_tsit5!(")
