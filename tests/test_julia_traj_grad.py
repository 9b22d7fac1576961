"""Textual check of the trajectory-ensemble gradient wrapper of julia/KANODEHip.jl against include/kanode.h (Julia is
not in this image, so the shim is not executed), in the manner of tests/test_julia_trajectories.py: the ccall names the
new symbol with the header's argument count, and the wrapper checks its sizes and the coverage before the call."""
import re

from test_julia_ensemble_solve import ccall_types, header_args
from test_julia_shim import JL, _functions, _strip


def test_ccalls_carry_the_headers_argument_count():
    c = header_args("kanode_trajectories_gradient_tsit5")
    j = ccall_types("kanode_trajectories_gradient_tsit5")
    assert len(c) == len(j) == 20, (c, j)
    # the scalar arguments line up by type
    for ca, ja in zip(c, j):
        if ca.startswith("int64_t "):
            assert ja == "Int64", (ca, ja)
        elif ca.startswith("double "):
            assert ja == "Float64", (ca, ja)
        else:
            assert ja.startswith(("Ptr{", "Ref{")), (ca, ja)
    assert c[10] == "double* loss" and j[10] == "Ref{Float64}"
    assert header_args("kanode_trajectories_gradient_supported") == ["const kanode_handle* h"]
    assert re.search(r"ccall\(sym\(:kanode_trajectories_gradient_supported\),\s*Int32,\s*\(Ptr\{Cvoid\},\),\s*h\.ptr\)",
                     JL)


def test_wrapper_checks_sizes_and_coverage_before_the_call():
    body = _functions(_strip(JL))["trajectories_gradient"][0]
    assert "u0::AbstractMatrix" in body and "p::AbstractVector" in body
    call = body.index(":kanode_trajectories_gradient_tsit5")
    for must in ("checkp(h, p)", "checku(h, u0", "h.nin == h.nout", "T == Float64", "1 <= R <= 65536",
                 "size(target) == (h.nin, R, length(ts))", "DimensionMismatch", "trajectories_gradient_supported(h)",
                 "ArgumentError", "issorted(ts)"):
        assert must in body and body.index(must) < call, must
    # the rows come back as [P, R]: C's [R][P] in Julia's column-major order
    assert "zeros(T, h.P, R)" in body
    assert re.search(r"trajectories_gradient_supported\(h::Handle\)", JL)
