"""The case table and the bar of the Fisher-KPP table-kernel parity matrix, checked on the CPU (tests/fk_table_cases.py;
numpy and the C oracle only, no kernel): every record's hand-stated launch equals the restated launch rules, the
coverage the matrix is there for is counted, the chosen inputs meet the conditions under which each wrong restatement
is visible, the scale is sound (the float64 numpy model against the C oracle stays far inside it on every record) and
it discriminates (eight wrong restatements of the kernels leave it on every record of their class and change nothing
where they cannot occur).

Measured here, worst err/bound of the float64 numpy model against the fp64 C oracle over the 873 single-launch records:
du 0.0025, λᵀJ 0.0025, dp 0.047 (asserted with a factor 3 to 4 of headroom).  Least err/bound of each wrong
restatement over its class, and the class size: see MUTATION_LEAST."""
import functools

import numpy as np
import pytest

import fk_cases as FC
import fk_table_cases as TC
from gpu_util import assert_close

RTOL = 1e-13
BY_ID = {c.id: c for c in TC.CASES}
SOLVE_BY_ID = {c.id: c for c in TC.SOLVE_CASES}


@pytest.fixture(scope="module", autouse=True)
def _drop_references():
    """The references are computed once and shared by this module's tests; they are let go when it ends."""
    yield
    _ref.cache_clear()


@functools.lru_cache(maxsize=None)
def _ref(cid):
    """(data, reference) of a record, read-only; a big pair record's reference is its slice's."""
    c = BY_ID[cid]
    d = c.data()
    r = TC.reference(c, d, TC.big_slice(c) if c.B == "big" else None)
    for a in list(vars(d).values()) + list(vars(r).values()):
        for x in (a if isinstance(a, list) else [a]):
            if isinstance(x, np.ndarray):
                x.setflags(write=False)
    return d, r


def _each(gid, check):
    """check(record) on every record of the group; every failing record is reported by its id."""
    failed = []
    for c in TC.GROUPS[gid]:
        try:
            check(c)
        except AssertionError as e:
            failed.append(f"{c.id}: {str(e).splitlines()[0] if str(e) else 'assert'}")
    assert not failed, f"{len(failed)} of {len(TC.GROUPS[gid])} records: " + "; ".join(failed[:8])


def _ratio(got, ref, scale):
    return float(np.max(np.abs(np.asarray(got, np.float64) - ref) / (RTOL * scale)))


def test_table_is_complete():
    assert len(BY_ID) == len(TC.CASES) == 873 and len(SOLVE_BY_ID) == len(TC.SOLVE_CASES) == 32
    assert sum(len(g) for g in TC.GROUPS.values()) == 873 and len(TC.GROUPS) == 24
    small = [c for c in TC.CASES if c.B != "big"]
    for diff in ("D0", "Ddx2"):                 # every shape, variant and option set exists at both
        a = {(c.op, c.variant, c.nx, c.B, c.opts) for c in small if c.diff == diff}
        assert a == {(c.op, c.variant, c.nx, c.B, c.opts) for c in small}
    assert {c.D_dx[0] for c in TC.CASES if c.diff == "D0"} == {0.0}
    for c in TC.CASES:                          # D = dx²: the Laplacian coefficient is 1
        if c.diff == "Ddx2":
            assert abs(TC._lap_co(c) - 1.0) < 1e-12
    have = {(c.op, c.nx, c.B, c.opts) for c in TC.CASES}
    for nx in (128, 256, 512):                  # the issue's lists
        for B in (1, 3, 4, 5, 15, 16, 17, 33):
            assert ("rhs", nx, B, ()) in have
        for B in (9, 13):
            for g in (1, 2):
                assert ("rhs", nx, B, (("grid_rhs", g),)) in have
        for B in (1, 4, 5, 9):
            assert ("stage", nx, B, ()) in have
        assert ("stage", nx, 9, (("grid_rhs", 1),)) in have
        for op in ("vjp", "vjp_stage"):
            for B in (1, 5, 31, 32, 33, 65):
                assert (op, nx, B, ()) in have
            for g in (1, 2):
                assert (op, nx, 9, (("grid_vjp", g),)) in have
    for nx in (2, 4, 6, 26, 64, 130, 510, 514, 1024):
        assert ("rhs", nx, 1, ()) in have and ("rhs", nx, 5, ()) in have
    assert {c.nx for c in TC.CASES if c.B == "big"} == {2, 26, 514}
    assert {(c.nx, c.B) for c in TC.SOLVE_CASES} >= {(nx, B) for nx in (128, 256, 512) for B in (1, 5)}


@pytest.mark.parametrize("gid", list(TC.GROUPS))
def test_record_states_its_launch(gid):
    """The hand-stated launch against the restated rules; the variant's path, table size and VJP support."""
    _each(gid, _states_its_launch)


def _states_its_launch(c):
    n, b, G, ni, nc, path, vjp = TC.VARIANTS[c.variant]
    assert TC.restated_launch(c).astuple() == c.launch.astuple()
    assert TC.make_ni(G, n)[0] == ni and TC.norm_class(n, b) == nc == c.launch.norm
    assert FC.fk_path("f64", c.spec()) == path
    assert TC.vjp_supported(c.variant, c.nx) == (vjp and c.nx in TC.NP_OF)
    if c.op in ("vjp", "vjp_stage"):
        assert vjp and FC.fk_path("f64", c.spec()) == c.launch.path and c.launch.gt == G
    if c.launch.family.startswith("pair"):
        fam, tl = TC.PAIR[c.nx]
        assert FC.fk_launch_class(c.nx) == ("pair", "short" if fam == "pair_short" else "long", tl)


def test_solve_records_state_their_launches():
    for c in TC.SOLVE_CASES:
        assert TC.restated_solve_launch(c) == (c.fwd, c.adj), c.id


def test_coverage_counts():
    L = [c.launch for c in TC.CASES] + [c.fwd for c in TC.SOLVE_CASES] + [c.adj for c in TC.SOLVE_CASES if c.adj]
    assert {l.family for l in L} == {"pair_short", "pair_long", "wave_rhs", "stage", "step", "step_loop", "vjp",
                                     "vjp_stage", "adj_step_rows", "adj_step_wave", "adj_loop"}
    for fam in ("wave_rhs", "stage", "step", "step_loop", "vjp", "vjp_stage", "adj_step_wave"):
        assert {l.np for l in L if l.family == fam} == {1, 2, 4}, fam
    for fam in ("adj_step_rows", "adj_loop"):
        assert {l.np for l in L if l.family == fam} == {1, 2}, fam
    for fam in ("pair_short", "pair_long", "wave_rhs", "stage", "step"):
        assert {l.norm for l in L if l.family == fam} == {"softsign", "tanh_fast", "runtime"}, fam
    for fam in ("vjp", "vjp_stage", "adj_step_rows"):
        assert {(l.norm, l.path, l.gt) for l in L if l.family == fam} >= {
            ("softsign", TC.REC_CORR, 10), ("softsign", TC.REC, 5), ("tanh_fast", TC.REC, 5)}, fam
    assert {(l.norm, l.path, l.gt) for l in L if l.family == "vjp"} == {
        ("softsign", TC.REC_CORR, 10), ("softsign", TC.REC, 5), ("tanh_fast", TC.REC_CORR, 10),
        ("tanh_fast", TC.REC, 5)}
    # NI = 256 at compile time and the runtime-ni kernel, both at the headline shape
    for fam in ("vjp", "adj_step_rows"):
        assert {l.ni256 for l in L if l.family == fam and l.np == 2} == {True, False}, fam
    assert any(c.nx == 256 and c.G == 5 and not c.launch.ni256 for c in TC.CASES if c.op == "vjp")
    assert {c.ni for c in TC.CASES if c.launch.family == "wave_rhs"} == {128, 256, 512}
    # rows-per-block tails of exactly one, full and full plus one, for both chunked kernels
    for op, per in (("rhs", 16), ("vjp", 32)):
        Bs = {c.B for c in TC.CASES if c.op == op and c.rows_per_block() == per}
        assert {1, per - 1, per, per + 1, 2 * per + 1} <= Bs, (op, Bs)
    # a second (and a ragged last) trip of a persistent grid, in every wave family that has one
    for op in ("rhs", "stage", "vjp", "vjp_stage"):
        trips = [c.trip_of() for c in TC.CASES if c.op == op and c.nx in TC.NP_OF and not c.launch.chunk]
        assert any(t.max() >= 2 and np.sum(t == t.max()) < TC.WPB for t in trips), op
    for (B, g), (grid, trips) in TC.WAVE_PERSIST.items():
        c = BY_ID[f"rhs-softsign_G10-nx128-B{B}-D0-grid_rhs{g}"]
        assert c.launch.grid == grid and int(c.trip_of().max()) + 1 == trips
    # the pair kernels' second trips: the unrolled two-row trip and a remainder (three trips' worth of rows)
    for c in TC.CASES:
        if c.B == "big":
            t = c.trip_of()
            assert t.max() == 2 and 0 < np.sum(t == 2) <= TC.pair_tpb(c.nx) + 1
            assert set(t[TC.big_slice(c)]) == {0, 1, 2}
            assert c.rows() * c.nx * 8 < 10 << 20
    # both sides of P + 1 workgroups, at G = 10 and G = 5
    for G in (10, 5):
        s = {(c.adj.grid - (G + 2), c.adj.fused_finish) for c in TC.SOLVE_CASES
             if c.opt.get("adj_fused_finish") and c.G == G}
        assert s == {(0, True), (-1, False)}
    # the integrator's option sets
    opts = {c.opts for c in TC.SOLVE_CASES}
    assert {(), (("fk_device_loop", 0),), (("adj_step_rows", 0),), (("fused_step", 0),)} <= opts
    assert any(c.adj is None and c.fwd.norm == "runtime" and c.nx == 128 for c in TC.SOLVE_CASES)
    assert {(c.nx, c.G) for c in TC.SOLVE_CASES} >= {(128, 5), (512, 5)}


@pytest.mark.parametrize("gid", list(TC.GROUPS))
def test_inputs_meet_the_conditions(gid):
    """What the wrong restatements need to be visible: every row differs from every other (in u and in λ), the stage
    arrays and coefficients are not zero, the planted points are there, no input is non-finite."""
    _each(gid, _meets_the_conditions)


def _meets_the_conditions(c):
    d = c.data()
    B = c.rows()
    assert d.u.shape == d.lam.shape == (B, c.nx)
    for a in (d.u, d.lam):
        assert np.isfinite(a).all()
        if B <= 65:
            assert len({r.tobytes() for r in a}) == B
            assert all(np.all(a[i] != a[j]) for i in range(B) for j in range(i + 1, min(B, i + 5)))
    if c.op in ("rhs", "vjp") and d.u.size >= 6:
        assert all(v in d.u for v in (0.0, 1e4, -1e4, 4.0, -4.0))
    if c.op in ("stage", "vjp_stage"):
        assert len(d.ks) == len(TC.STAGE_C) and all(TC.STAGE_C) and all(np.all(k != 0) for k in d.ks)
    if c.op == "vjp_stage":
        assert len(d.lks) == len(TC.LSTAGE_C) and all(TC.LSTAGE_C) and all(TC.STAGE_EC)
        _, r = _ref(c.id)
        assert np.mean(np.abs(r.ls) > 1.05 * np.abs(d.lam)) > 0.2      # err_scaled_by_lam has something to miss


# worst err/bound asserted (du, λᵀJ, dp): the module docstring's measured figures with headroom
SOUND = (0.01, 0.01, 0.15)


@pytest.mark.parametrize("gid", list(TC.GROUPS))
def test_scale_is_sound(gid):
    """The float64 numpy model (oracle/kanode_np.py's layer with fk_cases' Laplacian) against the C oracle at the point
    each record's RHS is taken at, under the record's own scale."""
    _each(gid, _scale_is_sound)


def _scale_is_sound(c):
    d, r = _ref(c.id)
    rows = TC.big_slice(c) if c.B == "big" else slice(None)
    y = getattr(r, "y", d.u[rows])
    ls = getattr(r, "ls", d.lam[rows])
    du, lamJ, dp = FC.np_fk(c, d.p, y, ls)
    if c.op in ("rhs", "stage"):
        assert_close(du, r.du, r.s_du, RTOL * SOUND[0], "numpy du")
    else:
        assert_close(lamJ, r.lamJ, r.s_lamJ, RTOL * SOUND[1], "numpy lamJ")
        assert_close(dp, r.dp, r.s_dp, RTOL * SOUND[2], "numpy dp")
    if c.op in ("stage", "vjp_stage"):
        assert 0 < r.err_bound < 1e-9 * r.err       # the derived bound is far tighter than the 1e-10..1e-9 in use


# least err/bound over the class, as measured (asserted with a factor 2 of slack), and the class size
MUTATION_LEAST = {
    "wrap_same_segment": (1.2e11, 254), "swap_um_up": (3.6e10, 381), "stale_last_row": (1.3e11, 762),
    "slipped_pipeline": (6.5e11, 450), "generic_small": (2.2e12, 6), "dp_less_a_block": (3.7e9, 216),
    "stage_less_last_k": (3.3e9, 282), "err_scaled_by_lam": (8.1e11, 192),
}


def _mut_ratio(c, d, r, which):
    got = TC.mutate(c, d, r, which)
    out = []
    for k, g in got.items():
        if k == "err":
            out.append(abs(g - r.err) / r.err_bound)
        else:
            out.append(_ratio(g, getattr(r, k), getattr(r, "s_" + k)))
    return max(out)


@pytest.mark.parametrize("which", list(TC.MUTATIONS))
def test_discrimination(which):
    """Every wrong restatement leaves the bar (err/bound > 1) on every record of its class, and equals the reference
    exactly on the records where it cannot occur."""
    group = [c for c in TC.CASES if TC.MUTATIONS[which](c)]
    least, missed = np.inf, {}
    for c in group:
        d, r = _ref(c.id)
        q = _mut_ratio(c, d, r, which)
        least = min(least, q)
        if not q > 1.0:
            missed[c.id] = q
    print(f"{which}: least err/bound {least:.3g} over {len(group)} records")
    assert len(group) == MUTATION_LEAST[which][1]
    assert not missed, f"{which}: not told from the oracle in {len(missed)} of {len(group)} records: {missed}"
    assert least >= MUTATION_LEAST[which][0] / 2
    if which in TC.CANNOT:
        never = [c for c in TC.CASES if TC.CANNOT[which](c)]
        assert never
        for c in never:
            d, r = _ref(c.id)
            for k, g in TC.mutate(c, d, r, which).items():
                assert np.array_equal(g, getattr(r, k)), (which, c.id)
