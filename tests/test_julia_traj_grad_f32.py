"""Textual check of the fp32 trajectory-ensemble gradient wrapper of julia/KANODEHip.jl against include/kanode.h (Julia
is not in this image, so the shim is not executed), in the manner of tests/test_julia_traj_grad.py: the ccall names the
new symbol with the header's argument count, the wrapper checks its sizes and the coverage before the call, and the
Float64 function is left as it was."""
import re

from test_julia_ensemble_solve import ccall_types, header_args
from test_julia_shim import JL, _functions, _strip


def test_ccalls_carry_the_headers_argument_count():
    c = header_args("kanode_trajectories_gradient_f32_tsit5")
    j = ccall_types("kanode_trajectories_gradient_f32_tsit5")
    assert len(c) == len(j) == 20, (c, j)
    for ca, ja in zip(c, j):
        if ca.startswith("int64_t "):
            assert ja == "Int64", (ca, ja)
        elif ca.startswith("double "):
            assert ja == "Float64", (ca, ja)
        else:
            assert ja.startswith(("Ptr{", "Ref{")), (ca, ja)
    assert c[10] == "double* loss" and j[10] == "Ref{Float64}"
    # argument for argument the fp64 entry
    assert c == header_args("kanode_trajectories_gradient_tsit5")
    assert j == ccall_types("kanode_trajectories_gradient_tsit5")
    assert header_args("kanode_trajectories_gradient_f32_supported") == ["const kanode_handle* h"]
    assert re.search(r"ccall\(sym\(:kanode_trajectories_gradient_f32_supported\),\s*Int32,\s*\(Ptr\{Cvoid\},\),"
                     r"\s*h\.ptr\)", JL)


def test_wrapper_checks_sizes_and_coverage_before_the_call():
    fns = _functions(_strip(JL))
    body = fns["trajectories_gradient_f32"][0]
    assert "u0::AbstractMatrix" in body and "p::AbstractVector" in body
    call = body.index(":kanode_trajectories_gradient_f32_tsit5")
    for must in ("checkp(h, p)", "checku(h, u0", "h.nin == h.nout", "T == Float32", "1 <= R <= 65536",
                 "size(target) == (h.nin, R, length(ts))", "DimensionMismatch",
                 "trajectories_gradient_f32_supported(h)", "ArgumentError", "issorted(ts)"):
        assert must in body and body.index(must) < call, must
    assert "zeros(T, h.P, R)" in body
    assert re.search(r"trajectories_gradient_f32_supported\(h::Handle\)", JL)
    # the Float64 function: one method, Float64 only, on the fp64 symbol
    assert len(fns["trajectories_gradient"]) == 1
    f64 = fns["trajectories_gradient"][0]
    assert "T == Float64" in f64 and ":kanode_trajectories_gradient_tsit5" in f64 and "_f32" not in f64
