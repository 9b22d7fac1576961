"""Textual check of the ensemble-solve wrappers of julia/KANODEHip.jl against include/kanode.h (Julia is not in this
image, so the shim is not executed), in the manner of tests/test_julia_shim.py: each ccall names the new symbol with
the header's argument count, and the wrapper checks its sizes and the coverage before the call."""
import re

from test_julia_shim import HDR, JL, _functions, _strip


def header_args(name):
    decl = re.search(r"\b" + name + r"\s*\((.*?)\)\s*;", HDR, flags=re.S).group(1)
    return [a.strip() for a in decl.split(",")]


def ccall_types(name):
    """The argument-type tuple of the ccall of `name`."""
    m = re.search(r"ccall\(sym\(:" + name + r"\),\s*\w+,\s*\((.*?)\)\s*,\s*\n?\s*h\.ptr", JL, flags=re.S)
    assert m, name
    depth, parts, cur = 0, [], ""
    for ch in m.group(1):
        if ch in "{(":
            depth += 1
        if ch in "})":
            depth -= 1
        if ch == "," and depth == 0:
            parts.append(cur.strip())
            cur = ""
        else:
            cur += ch
    return parts + ([cur.strip()] if cur.strip() else [])


def test_ccalls_carry_the_headers_argument_count():
    c = header_args("kanode_solve_ensemble_tsit5")
    j = ccall_types("kanode_solve_ensemble_tsit5")
    assert len(c) == len(j) == 14, (c, j)
    # the scalar arguments line up by type
    for ca, ja in zip(c, j):
        if ca.startswith("int64_t "):
            assert ja == "Int64", (ca, ja)
        elif ca.startswith("double "):
            assert ja == "Float64", (ca, ja)
        else:
            assert ja.startswith(("Ptr{", "Ref{")), (ca, ja)
    assert header_args("kanode_solve_ensemble_supported") == ["const kanode_handle* h", "int64_t batch"]
    assert ccall_types("kanode_solve_ensemble_supported") == ["Ptr{Cvoid}", "Int64"]


def test_wrapper_checks_sizes_and_coverage_before_the_call():
    body = _functions(_strip(JL))["solve_ensemble_tsit5"][0]
    assert "ps::AbstractMatrix" in body
    call = body.index(":kanode_solve_ensemble_tsit5")
    for must in ("size(ps, 1) == h.P", "DimensionMismatch", "checku(h, u0", "solve_ensemble_supported(h, B)",
                 "ArgumentError", "issorted(ts)"):
        assert must in body and body.index(must) < call, must
    assert re.search(r"solve_ensemble_supported\(h::Handle, B::Integer\)", JL)
