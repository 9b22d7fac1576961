"""Textual check of the trajectory-ensemble wrappers of julia/KANODEHip.jl against include/kanode.h (Julia is not in
this image, so the shim is not executed), in the manner of tests/test_julia_ensemble_solve.py: each ccall names the new
symbol with the header's argument count, and the wrapper checks its sizes and the coverage before the call."""
import re

from test_julia_ensemble_solve import ccall_types, header_args
from test_julia_shim import JL, _functions, _strip


def test_ccalls_carry_the_headers_argument_count():
    c = header_args("kanode_solve_trajectories_tsit5")
    j = ccall_types("kanode_solve_trajectories_tsit5")
    assert len(c) == len(j) == 13, (c, j)
    # the scalar arguments line up by type
    for ca, ja in zip(c, j):
        if ca.startswith("int64_t "):
            assert ja == "Int64", (ca, ja)
        elif ca.startswith("double "):
            assert ja == "Float64", (ca, ja)
        else:
            assert ja.startswith(("Ptr{", "Ref{")), (ca, ja)
    assert header_args("kanode_solve_trajectories_supported") == ["const kanode_handle* h"]
    assert re.search(r"ccall\(sym\(:kanode_solve_trajectories_supported\),\s*Int32,\s*\(Ptr\{Cvoid\},\),\s*h\.ptr\)", JL)


def test_wrapper_checks_sizes_and_coverage_before_the_call():
    body = _functions(_strip(JL))["solve_trajectories"][0]
    assert "u0::AbstractMatrix" in body and "p::AbstractVector" in body
    call = body.index(":kanode_solve_trajectories_tsit5")
    for must in ("checkp(h, p)", "checku(h, u0", "h.nin == h.nout", "1 <= R <= 65536", "solve_trajectories_supported(h)",
                 "ArgumentError", "issorted(ts)"):
        assert must in body and body.index(must) < call, must
    # the result has the batched solve's layout: [N, R, n_save] in Julia's column-major order is C's [n_save][R][N]
    assert "fill(T(NaN), h.nin, R, length(ts))" in body
    assert re.search(r"solve_trajectories_supported\(h::Handle\)", JL)
