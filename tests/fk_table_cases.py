"""The cases the parity matrix of the Fisher-KPP TABLE kernels shares (test_fk_table_cases_cpu.py,
test_gpu_fk_table_matrix.py): the records, the kernel family and launch each record is meant to reach (kan_pp.hip:
fk_rhs_pp_kernel, fk_rhs_pp_wave_kernel, fk_stage_pp_wave_kernel, fk_step_pp_wave_kernel, fk_vjp_pp_wave_kernel,
fk_vjp_step_rows_kernel, fk_vjp_step_pp_wave_kernel and the two device loops, behind the launch_fk_*_pp launchers),
stated by hand as the record kanode_last_fk_launch must return; the seeded inputs; the error scale; the launch rules
restated; and the wrong restatements the CPU test holds against the oracle.  No tests live here.

The pass criterion of a single-launch record is gpu_util.assert_close(got, ref, scale, RTOL[float64]).  The scale is
fk_cases.fk_error_scale at the point the RHS is taken at, plus the table's own documented tolerance: an interval is
accepted when its check points are within pc.tol = 2e-14 of their Σ|terms| floored by the function's magnitude
(kan_pp_build.hpp), which the arithmetic scale has no term for.  In units of RTOL = 1e-13 that is 0.2 of
Σ|C_j| + |W||u| for du (the scale test_gpu_pp.py holds at 1e-14), 0.2·|λ|·(invh·Σ|C_j| + |W|) for λᵀJ (the φ'
table's magnitude) and 0.2·Σ|λ|(1 + |u|) for dW (the swish table's); dC takes no table.  table_term() is the one
place it is added.

The restated rules (wave_launch, pair_launch, stage_launch, vjp_launch, adj_step_launch, make_ni) can drift from the
C++: the records state their launches by hand, the CPU test holds them against these restatements, and the GPU
matrix holds the same statements against the library's own record."""
from __future__ import annotations

import zlib
from dataclasses import dataclass
from types import SimpleNamespace

import numpy as np

import fk_cases as FC
from oracle import kanode_np as N
from oracle import oracle as O

REC, REC_CORR = FC.REC, FC.REC_CORR
K_BLOCK, K_WAVE, K_SLAB = 256, 64, 4096        # kan_common.hpp, kanode_options.hpp
RHS_CHUNK, VJP_CHUNK = 4, 8                    # kan_pp.hip: KAN_PP_CHUNK, KAN_VJP_CHUNK
WPB = K_BLOCK // K_WAVE                        # waves (rows in flight) per block of every wave kernel
NOMINAL_CUS = 256                              # the MI355X; a GPU run takes the device's own count
PAD = 32                                       # NaN rows behind every input and output (a whole VJP block)

# name: (normalizer, basis, G, ni, the kernels' normalizer class, PATH in fp64, the table VJP covers it)
VARIANTS = {
    "softsign_G10": ("softsign", "rbf", 10, 256, "softsign", REC_CORR, True),
    "softsign_G5": ("softsign", "rbf", 5, 128, "softsign", REC, True),
    "tanhfast_G10": ("tanh_fast", "rbf", 10, 256, "tanh_fast", REC_CORR, True),
    "tanhfast_G5": ("tanh_fast", "rbf", 5, 128, "tanh_fast", REC, True),
    "tanh_G5": ("tanh", "rbf", 5, 128, "runtime", REC, False),             # NORM_RUNTIME, BASIS -1
    "softsign_rswaf_G5": ("softsign", "rswaf", 5, 128, "runtime", FC.DIRECT, False),
    "softsign_G16": ("softsign", "rbf", 16, 512, "softsign", REC_CORR, False),   # w = 1/64: the largest table
}
TABLE_VJP = ["softsign_G10", "softsign_G5", "tanhfast_G10", "tanhfast_G5"]
WAVE_VARIANTS = ["softsign_G10", "tanhfast_G5", "tanh_G5", "softsign_G16"]
PAIR_VARIANTS = ["softsign_G10", "tanhfast_G5", "softsign_rswaf_G5"]
STAGE_VARIANTS = ["softsign_G10", "tanhfast_G5", "tanh_G5"]

NP_OF = {128: 1, 256: 2, 512: 4}
# ---- launches, stated by hand --------------------------------------------------------------------------------------
# wave RHS, default: 4 waves x chunk 4 = 16 rows per block, the grid covers the batch
WAVE_GRID = {1: 1, 3: 1, 4: 1, 5: 1, 15: 1, 16: 1, 17: 2, 33: 3}
# wave RHS, KANODE_OPT_GRID_RHS = g: chunk 0, the grid strides; (B, g) -> (grid, trips of wave 0)
WAVE_PERSIST = {(9, 1): (1, 3), (9, 2): (2, 2), (13, 1): (1, 4), (13, 2): (2, 2)}
# pair kernels: nx -> (family, tpt_log2); (nx, B) -> grid
PAIR = {2: ("pair_short", 0), 4: ("pair_short", 1), 6: ("pair_short", 2), 26: ("pair_short", 4),
        64: ("pair_short", 5), 130: ("pair_short", 7), 510: ("pair_short", 8), 514: ("pair_long", 8),
        1024: ("pair_long", 8)}
PAIR_GRID = {(2, 1): 1, (2, 5): 1, (4, 1): 1, (4, 5): 1, (6, 1): 1, (6, 5): 1, (26, 1): 1, (26, 5): 1, (64, 1): 1,
             (64, 5): 1, (130, 1): 1, (130, 5): 3, (510, 1): 1, (510, 5): 5, (514, 1): 1, (514, 5): 5, (1024, 1): 1,
             (1024, 5): 5}
PAIR_BIG_NX = (2, 26, 514)     # B = 2·tpb·cap + tpb + 1, grid = cap = 4 x CUs
# stage: one row per wave, always the persistent form; B -> grid (and with grid_rhs = 1)
STAGE_GRID = {1: 1, 4: 1, 5: 2, 9: 3}
# standalone VJP, default: 4 waves x chunk 8 = 32 rows per block
VJP_GRID = {1: 1, 5: 1, 31: 1, 32: 1, 33: 2, 65: 3}
# VJP stage: one row per wave, persistent
VJP_STAGE_GRID = {1: 1, 5: 2, 31: 8, 32: 8, 33: 9, 65: 17}


@dataclass(frozen=True)
class Launch:
    """What kanode_last_fk_launch must say (KanodeHandle.last_fk_launch's FkLaunch, field for field)."""
    family: str
    np: int
    norm: str
    path: str | None = None
    gt: int = 0
    ni256: bool = False
    chunk: int = 0
    grid: int | str = 1          # "cap": 4 x the device's CU count
    combine: int = 0
    fused_finish: bool = False

    def astuple(self, cus=NOMINAL_CUS):
        g = 4 * cus if self.grid == "cap" else self.grid
        return (self.family, self.np, self.norm, self.path, self.gt, self.ni256, self.chunk, g, self.combine,
                self.fused_finish)


# ---- the rules, restated (kan_pp.hip launch_fk_*_pp; kanode_abi.cpp make_pp_const) ---------------------------------
def make_ni(G, normalizer="softsign", lims=(-1.0, 1.0)):
    """make_pp_const's interval count: w the largest power of two <= min(1/16, 0.16·h_u), h_u = 1/invh (x 4 for a
    sigmoid); ni the largest power of two <= 512 with ni·w <= 8."""
    invh = float(N.inv_h(N.default_denominator(G)))
    hu = (1.0 / invh) / (0.25 if normalizer.startswith("sigmoid") else 1.0)
    w = 1.0 / 16.0
    while w > 0.16 * hu and w > 2.0 ** -20:
        w *= 0.5
    ni = 512
    while ni > 16 and ni * w > 8.0:
        ni >>= 1
    return ni, w


def norm_class(normalizer, basis):
    return normalizer if basis == "rbf" and normalizer in ("softsign", "tanh_fast") else "runtime"


def grid_for(work, per_block, cap):
    return max(1, min((work + per_block - 1) // per_block, cap))


def rhs_launch(variant, nx, B, grid_rhs=0, cus=NOMINAL_CUS):
    """launch_fk_rhs_pp: the wave kernel at nx = 128, 256, 512 (chunk 4 over a batch-covering grid, or chunk 0 under
    a grid override), else the pair kernels: short while nx/2 <= kBlock, tpb = kBlock >> ceil_log2(min(nx/2,
    kBlock)) trajectories per block, the grid capped at 4 x CUs."""
    n, b = VARIANTS[variant][:2]
    nc = norm_class(n, b)
    if nx in NP_OF:
        if grid_rhs > 0:
            return Launch("wave_rhs", NP_OF[nx], nc, chunk=0, grid=grid_for(B, WPB, grid_rhs))
        return Launch("wave_rhs", NP_OF[nx], nc, chunk=RHS_CHUNK, grid=grid_for(B, WPB * RHS_CHUNK, 1 << 30))
    units = nx // 2
    tl = FC.fk_launch_class(nx)[2]
    g = grid_for(B, K_BLOCK >> tl, 4 * cus)
    return Launch("pair_short" if units <= K_BLOCK else "pair_long", 0, nc, grid="cap" if g == 4 * cus else g)


def pair_tpb(nx):
    return K_BLOCK >> FC.fk_launch_class(nx)[2]


def pair_big_B(nx, cus=NOMINAL_CUS):
    """The batch that takes the two-row unrolled trip of SHORT and then a remainder trip (three trips of the long
    kernel's loop): 2·tpb·cap + tpb + 1."""
    return 2 * pair_tpb(nx) * 4 * cus + pair_tpb(nx) + 1


def stage_launch(variant, nx, B, grid_rhs=0, cus=NOMINAL_CUS):
    n, b = VARIANTS[variant][:2]
    cap = grid_rhs if grid_rhs > 0 else 4 * cus
    return Launch("stage", NP_OF[nx], norm_class(n, b), grid=grid_for(B, WPB, min(cap, K_SLAB)))


def vjp_supported(variant, nx):
    n, b, G, _, _, path, _ = VARIANTS[variant]
    return nx in NP_OF and b == "rbf" and path != FC.DIRECT and G in (5, 10) and n in ("softsign", "tanh_fast")


def vjp_launch(variant, nx, B, stage, grid_vjp=0, cus=NOMINAL_CUS):
    """fk_vjp_pp_go: the standalone VJP takes contiguous chunks (8 rows per wave, doubled until the grid fits the
    slab) unless a grid override makes it persistent; the stage form is always persistent, its slab cap halved.  The
    compile-time NI = 256 kernel serves the standalone VJP at nx = 256 alone."""
    assert vjp_supported(variant, nx)
    n, _, G, ni, nc, path, _ = VARIANTS[variant]
    if not stage and grid_vjp == 0:
        chunk = VJP_CHUNK
        while (B + WPB * chunk - 1) // (WPB * chunk) > K_SLAB:
            chunk *= 2
        grid = grid_for(B, WPB * chunk, K_SLAB)
    else:
        chunk = 0
        cap = grid_vjp if grid_vjp > 0 else 4 * cus
        grid = grid_for(B, WPB, min(cap, K_SLAB // 2 if stage else K_SLAB))
    return Launch("vjp_stage" if stage else "vjp", NP_OF[nx], nc, path, G, nx == 256 and not stage and ni == 256,
                  chunk, grid)


def adj_step_launch(variant, nx, B, adaptive, rows=1, grid_adj_step=0, fused_finish=0, device_loop=1):
    """launch_fk_vjp_step_pp / launch_fk_adjoint_loop: the rows kernel where asked, no grid override, nx <= 256 and
    one row per wave fits the slab (kSlabBlocks / 2 rows here); only it combines (1 fixed, 2 adaptive); the finish
    fuses on the combined adaptive step with at least P + 1 workgroups; the adaptive adjoint runs as the device loop
    where the rows kernel would serve it and the loop is on."""
    assert vjp_supported(variant, nx)
    n, _, G, ni, nc, path, _ = VARIANTS[variant]
    P = G + 1
    slab = K_SLAB // 2
    use_rows = bool(rows) and grid_adj_step == 0 and nx <= 256 and B <= WPB * slab
    grid = grid_for(B, WPB, slab if use_rows else min(grid_adj_step or 4 * NOMINAL_CUS, slab))
    if use_rows and adaptive and device_loop and not fused_finish:    # (kanode_fused.cpp: the loop declines the option)
        return Launch("adj_loop", NP_OF[nx], nc, path, G, nx == 256 and ni == 256, 0, grid, 2, False)
    combine = (2 if adaptive else 1) if use_rows else 0
    fused = bool(fused_finish) and combine == 2 and grid >= P + 1
    return Launch("adj_step_rows" if use_rows else "adj_step_wave", NP_OF[nx], nc, path, G,
                  use_rows and nx == 256 and ni == 256, 0, grid, combine, fused)


# ---- records -------------------------------------------------------------------------------------------------------
STAGE_C = (0.11, -0.07, 0.05, 0.13, -0.03, 0.02)            # c_j of the six stage arrays (none zero)
STAGE_EC = (0.003, -0.002, 0.004, 0.001, -0.005, 0.002, 0.006)
LSTAGE_C = (0.09, 0.04, -0.06, 0.12, 0.07, -0.05)
ABSTOL, RELTOL = 1e-6, 1e-3


@dataclass(frozen=True)
class Case:
    op: str            # "rhs", "stage", "vjp", "vjp_stage"
    variant: str
    nx: int
    B: int | str       # "big": pair_big_B(nx) of the device
    diff: str          # "D0" / "Ddx2" (fk_cases.DIFFUSION)
    launch: Launch
    opts: tuple = ()   # ((option, value), ...)

    @property
    def id(self):
        o = "".join(f"-{k}{v}" for k, v in self.opts)
        return f"{self.op}-{self.variant}-nx{self.nx}-B{self.B}-{self.diff}{o}"

    @property
    def seed(self):
        return zlib.crc32(self.id.encode())

    @property
    def G(self):
        return VARIANTS[self.variant][2]

    @property
    def use_base(self):
        return True

    @property
    def ni(self):
        return VARIANTS[self.variant][3]

    @property
    def path(self):
        return VARIANTS[self.variant][5]

    @property
    def D_dx(self):
        return FC.DIFFUSION[self.diff](self.nx)

    @property
    def opt(self):
        return dict(self.opts)

    def rows(self, cus=NOMINAL_CUS):
        return pair_big_B(self.nx, cus) if self.B == "big" else self.B

    def spec(self):
        n, b, G = VARIANTS[self.variant][:3]
        return O.LayerSpec(1, 1, G, n, b, True, (-1.0, 1.0), None, True)

    # -- how the rows fall on blocks and trips (for the coverage counts and the wrong restatements) --
    def rows_per_block(self):
        """Rows one block takes in one pass of its chunk (None: a persistent grid or a pair kernel)."""
        return WPB * self.launch.chunk if self.launch.chunk else None

    def block_of(self, cus=NOMINAL_CUS):
        """The block every row is computed by (wave kernels)."""
        B, r = self.rows(cus), np.arange(self.rows(cus))
        if self.launch.chunk:
            return r // (WPB * self.launch.chunk)
        return (r // WPB) % self.launch.astuple(cus)[7]

    def trip_of(self, cus=NOMINAL_CUS):
        """The trip of its wave's (pair kernels: its thread group's) row loop every row is computed in."""
        r = np.arange(self.rows(cus))
        g = self.launch.astuple(cus)[7]
        if self.launch.family.startswith("pair"):
            return r // (pair_tpb(self.nx) * g)
        if self.launch.chunk:
            return (r % (WPB * self.launch.chunk)) // WPB
        return r // (WPB * g)

    def data(self, cus=NOMINAL_CUS):
        """SimpleNamespace of float64 arrays: p (Glorot-uniform), u (uniform in [-3, 3]), lam (standard normal) and,
        for the stage forms, ks / lks (six arrays each, 0.3·normal / normal).  Planted into u at seeded places, as
        far as there is room: exactly 0, ±1e4 (off the table: the direct formula), 4.0 (the first point past the
        table) and -4.0 (its first point).  Every row is drawn independently, so no two are equal."""
        rng = np.random.default_rng(self.seed)
        B, G = self.rows(cus), self.G
        lim = np.sqrt(6.0 / (1 + G))
        p = np.concatenate([rng.uniform(-lim, lim, G), rng.uniform(-np.sqrt(3.0), np.sqrt(3.0), 1)])
        u = rng.uniform(-3.0, 3.0, (B, self.nx))
        lam = rng.normal(size=(B, self.nx))
        plant = [0.0, 1e4, -1e4, 4.0, -4.0]
        k = min(len(plant), u.size - 1)
        if k > 0 and self.op in ("rhs", "vjp"):     # (a stage point is a sum: nothing planted survives it)
            u.reshape(-1)[rng.choice(u.size, k, replace=False)] = plant[:k]
        d = SimpleNamespace(p=p, u=u, lam=lam)
        if self.op in ("stage", "vjp_stage"):
            d.ks = [0.3 * rng.normal(size=u.shape) for _ in STAGE_C]
        if self.op == "vjp_stage":
            d.lks = [rng.normal(size=u.shape) for _ in LSTAGE_C]
        return d


def _cases():
    out = []
    for diff in ("D0", "Ddx2"):
        for nx in (128, 256, 512):
            npp = NP_OF[nx]
            for v in WAVE_VARIANTS:
                nc = VARIANTS[v][4]
                for B, g in WAVE_GRID.items():
                    out.append(Case("rhs", v, nx, B, diff, Launch("wave_rhs", npp, nc, chunk=4, grid=g)))
                for (B, go), (g, _) in WAVE_PERSIST.items():
                    out.append(Case("rhs", v, nx, B, diff, Launch("wave_rhs", npp, nc, chunk=0, grid=g),
                                    (("grid_rhs", go),)))
            for v in STAGE_VARIANTS:
                nc = VARIANTS[v][4]
                for B, g in STAGE_GRID.items():
                    out.append(Case("stage", v, nx, B, diff, Launch("stage", npp, nc, grid=g)))
                out.append(Case("stage", v, nx, 9, diff, Launch("stage", npp, nc, grid=1), (("grid_rhs", 1),)))
            for v in TABLE_VJP:
                _, _, G, ni, nc, path, _ = VARIANTS[v]
                ct = nx == 256 and ni == 256      # the FK256 tables; (256, G = 5) takes the runtime-ni kernel
                for B, g in VJP_GRID.items():
                    out.append(Case("vjp", v, nx, B, diff, Launch("vjp", npp, nc, path, G, ct, 8, g)))
                for B, g in VJP_STAGE_GRID.items():
                    out.append(Case("vjp_stage", v, nx, B, diff, Launch("vjp_stage", npp, nc, path, G, False, 0, g)))
                for go in (1, 2):
                    out.append(Case("vjp", v, nx, 9, diff, Launch("vjp", npp, nc, path, G, ct, 0, go),
                                    (("grid_vjp", go),)))
                    out.append(Case("vjp_stage", v, nx, 9, diff,
                                    Launch("vjp_stage", npp, nc, path, G, False, 0, go), (("grid_vjp", go),)))
        for v in PAIR_VARIANTS:
            nc = VARIANTS[v][4]
            for nx, (fam, _) in PAIR.items():
                for B in (1, 5):
                    out.append(Case("rhs", v, nx, B, diff, Launch(fam, 0, nc, grid=PAIR_GRID[nx, B])))
    for nx in PAIR_BIG_NX:      # a few megabytes each: one variant, the Laplacian on
        out.append(Case("rhs", "softsign_G10", nx, "big", "Ddx2", Launch(PAIR[nx][0], 0, "softsign", grid="cap")))
    return out


CASES = _cases()
SINGLE_OPS = ("rhs", "stage", "vjp", "vjp_stage")


def _groups():
    """The records by operation and nx (a big pair record on its own): one test per group, so that the matrix adds
    tens of test ids, not thousands; a test goes through its group's records, reports every one that fails and
    names it."""
    out = {}
    for c in CASES:
        out.setdefault(f"{c.op}-nx{c.nx}" + ("-big" if c.B == "big" else ""), []).append(c)
    return out


GROUPS = _groups()


def restated_launch(c, cus=NOMINAL_CUS):
    B = c.rows(cus)
    if c.op == "rhs":
        return rhs_launch(c.variant, c.nx, B, c.opt.get("grid_rhs", 0), cus)
    if c.op == "stage":
        return stage_launch(c.variant, c.nx, B, c.opt.get("grid_rhs", 0), cus)
    return vjp_launch(c.variant, c.nx, B, c.op == "vjp_stage", c.opt.get("grid_vjp", 0), cus)


def big_slice(c, cus=NOMINAL_CUS):
    """Rows of a big pair record compared with the oracle: the first and last rows of every trip."""
    B = c.rows(cus)
    per = pair_tpb(c.nx) * 4 * cus
    rows = sorted({r for k in range(3) for r in (k * per, k * per + 1, min((k + 1) * per, B) - 1) if r < B})
    return np.array(rows)


# ---- the integrator records (the step and adjoint-step classes) ---------------------------------------------------
@dataclass(frozen=True)
class SolveCase:
    """One run of test_gpu_fk_e2e._e2e's form, shortened: 4 fixed steps, or its short adaptive span.  fwd / adj: the
    launch records after the forward solve and after the adjoint (adj None: the adjoint does not take the table VJP,
    so the forward's record is still the last)."""
    variant: str
    nx: int
    B: int
    mode: str          # "fixed" / "adaptive"
    fwd: Launch
    adj: Launch | None
    opts: tuple = ()

    @property
    def id(self):
        o = "".join(f"-{k}{v}" for k, v in self.opts)
        return f"solve-{self.variant}-nx{self.nx}-B{self.B}-{self.mode}{o}"

    @property
    def opt(self):
        return dict(self.opts)

    @property
    def G(self):
        return VARIANTS[self.variant][2]


def _step(v, nx, B, fam="step"):
    return Launch(fam, NP_OF[nx], VARIANTS[v][4], grid=(B + WPB - 1) // WPB)


def _adj(v, nx, B, fam, combine=0, fused=False):
    _, _, G, ni, nc, path, _ = VARIANTS[v]
    ct = fam in ("adj_step_rows", "adj_loop") and nx == 256 and ni == 256
    return Launch(fam, NP_OF[nx], nc, path, G, ct, 0, (B + WPB - 1) // WPB, combine, fused)


def _solve_cases():
    out = []
    S10 = "softsign_G10"
    for nx in (128, 256, 512):
        rows = nx <= 256
        for B in (1, 5):
            # the defaults: fixed steps combine through A (1); adaptive: both device loops where the rows kernel serves
            out.append(SolveCase(S10, nx, B, "fixed", _step(S10, nx, B),
                                 _adj(S10, nx, B, "adj_step_rows", 1) if rows else _adj(S10, nx, B, "adj_step_wave")))
            out.append(SolveCase(S10, nx, B, "adaptive", _step(S10, nx, B, "step_loop"),
                                 _adj(S10, nx, B, "adj_loop", 2) if rows else _adj(S10, nx, B, "adj_step_wave")))
        # the host-controlled adaptive step (error partials) and adjoint step (combine 2, finish as its own launch)
        out.append(SolveCase(S10, nx, 5, "adaptive", _step(S10, nx, 5),
                             _adj(S10, nx, 5, "adj_step_rows", 2) if rows else _adj(S10, nx, 5, "adj_step_wave"),
                             (("fk_device_loop", 0),)))
        # the stage launches in place of the fused step and of the fused adjoint step (both need fused_step)
        out.append(SolveCase(S10, nx, 5, "fixed", _step(S10, nx, 5, "stage"), _adj(S10, nx, 5, "vjp_stage"),
                             (("fused_step", 0),)))
    for nx in (128, 256):       # the wave adjoint step below its default size
        for mode in ("fixed", "adaptive"):
            out.append(SolveCase(S10, nx, 5, mode, _step(S10, nx, 5, "step" if mode == "fixed" else "step_loop"),
                                 _adj(S10, nx, 5, "adj_step_wave"), (("adj_step_rows", 0),)))
    # the fused finish on both sides of P + 1 workgroups (P = G + 1): B = 4(P + 1) fuses, 4(P + 1) - 4 must not
    for v, nx in (("softsign_G10", 256), ("softsign_G5", 128)):
        P = VARIANTS[v][2] + 1
        for B, fused in ((4 * (P + 1), True), (4 * (P + 1) - 4, False)):
            out.append(SolveCase(v, nx, B, "adaptive", _step(v, nx, B), _adj(v, nx, B, "adj_step_rows", 2, fused),
                                 (("adj_fused_finish", 1), ("fk_device_loop", 0))))
    # G = 5 (the runtime-ni kernels) at the two sizes the suite never ran it at.  Fixed steps at nx = 512: the short
    # adaptive span there takes its steps at Tsit5's stability limit (16 steps of 3.1e-4 against 3.3 / (4D/dx²) =
    # 3.2e-4), and with these parameters the oracle driver run twice, once with one-ulp noise on its own du, differs
    # from itself by 8.4e-12 (tanh_fast) and 9.6e-12 (softsign) in u: the 1e-11 bar would measure that, not the
    # kernels (the G = 10 records at nx = 512 above: 2.1e-13 under the same noise; nx = 256: 2.4e-15)
    for v in ("tanhfast_G5", "softsign_G5"):
        out.append(SolveCase(v, 128, 5, "fixed", _step(v, 128, 5), _adj(v, 128, 5, "adj_step_rows", 1)))
        out.append(SolveCase(v, 512, 5, "fixed", _step(v, 512, 5), _adj(v, 512, 5, "adj_step_wave")))
    # the rows kernel with the runtime-ni tables at the headline shape (NI = 256 is what every other record takes there)
    out.append(SolveCase("tanhfast_G5", 256, 5, "adaptive", _step("tanhfast_G5", 256, 5),
                         _adj("tanhfast_G5", 256, 5, "adj_step_rows", 2), (("fk_device_loop", 0),)))
    # a runtime-normalizer handle: the table step kernel forward, no table VJP backward
    out.append(SolveCase("tanh_G5", 128, 5, "fixed", _step("tanh_G5", 128, 5), None))
    return out


SOLVE_CASES = _solve_cases()


def restated_solve_launch(c):
    """(fwd, adj) from the restated rules."""
    o = c.opt
    adaptive = c.mode == "adaptive"
    loop = o.get("fk_device_loop", 1)
    if not o.get("fused_step", 1):
        fam = "stage"
    else:
        fam = "step_loop" if adaptive and loop else "step"
    fwd = Launch(fam, NP_OF[c.nx], VARIANTS[c.variant][4], grid=grid_for(c.B, WPB, 4 * NOMINAL_CUS))
    if not vjp_supported(c.variant, c.nx):
        return fwd, None
    if not o.get("fused_step", 1):
        return fwd, vjp_launch(c.variant, c.nx, c.B, True, o.get("grid_vjp", 0))
    return fwd, adj_step_launch(c.variant, c.nx, c.B, adaptive, o.get("adj_step_rows", 1), o.get("grid_adj_step", 0),
                                o.get("adj_fused_finish", 0), loop)


# ---- references and scales -----------------------------------------------------------------------------------------
def stage_point(base, ks, cs):
    """base + Σ c_j k_j, formed in extended precision and rounded once (the kernels' fma chains differ from it by
    at most len(ks) roundings of the sum's terms, which fk_error_scale's input term covers)."""
    y = np.asarray(base, np.longdouble)
    for c, k in zip(cs, ks):
        y = y + np.longdouble(c) * np.asarray(k, np.longdouble)
    return y.astype(np.float64)


def table_term(c, p, u, lam):
    """(du, λᵀJ, dp) terms of the table's acceptance tolerance, in units of RTOL (module docstring)."""
    G = c.G
    csum, W = float(np.sum(np.abs(p[:G]))), abs(float(p[G]))
    invh = float(N.inv_h(N.default_denominator(G)))
    f = 2e-14 / 1e-13
    dp = np.zeros(G + 1)
    dp[G] = f * float(np.sum(np.abs(lam) * (1.0 + np.abs(u))))
    return f * (csum + W * np.abs(u)), f * np.abs(lam) * (invh * csum + W), dp


def scales(c, p, u, lam):
    """(du, λᵀJ, dp) scales at the point u: fk_cases.fk_error_scale plus table_term."""
    s = FC.fk_error_scale(c, p, u, lam)
    t = table_term(c, p, u, lam)
    return tuple(a + b for a, b in zip(s, t))


def err_norm(ec, ks, last, a, b):
    """Σ (e / (abstol + reltol·max(|a|, |b|)))², e = Σ ec_j k_j + ec_last·last, and the bound on its error when
    `last` is known to dlast: (value, lambda dlast: bound).  The bound carries dlast through e and adds the roundings
    of e (one per term), of the quotient and square (3) and of the sum (a pairwise-or-better order: 64 roundings
    cover 10^5 points several times over)."""
    eps = np.finfo(np.float64).eps
    e = sum(cj * kj for cj, kj in zip(ec[:-1], ks)) + ec[-1] * last
    mag = sum(abs(cj) * np.abs(kj) for cj, kj in zip(ec[:-1], ks)) + abs(ec[-1]) * np.abs(last)
    sk = ABSTOL + RELTOL * np.maximum(np.abs(a), np.abs(b))
    r = e / sk
    val = float(np.sum(r * r))

    def bound(dlast):
        dr = (abs(ec[-1]) * dlast + (len(ec) + 1) * eps * mag) / sk + 3 * eps * np.abs(r)
        return float(np.sum(2 * np.abs(r) * dr + dr * dr)) + 64 * eps * val
    return val, bound


def reference(c, d, rows=None):
    """What the record's call must return, from the fp64 C oracle, and the scales: a SimpleNamespace of du | lamJ, dp
    (and y, ls, err for the stage forms) with s_<name> scales.  rows: only these rows (rhs)."""
    p = d.p
    u = d.u if rows is None else d.u[rows]
    lam = d.lam if rows is None else d.lam[rows]
    D, dx = c.D_dx
    r = SimpleNamespace()
    if c.op == "rhs":
        r.du = O.fk_rhs(c.spec(), p, D, dx, u)
        r.s_du = scales(c, p, u, lam)[0]
    elif c.op == "stage":
        r.y = stage_point(u, d.ks, STAGE_C)
        r.du = O.fk_rhs(c.spec(), p, D, dx, r.y)
        r.s_du = scales(c, p, r.y, lam)[0]
        r.err, r.err_bound = err_norm(STAGE_EC, d.ks, r.du, u, r.y)
        r.err_bound = r.err_bound(1e-13 * r.s_du)
    else:
        r.y = stage_point(u, d.ks, STAGE_C) if c.op == "vjp_stage" else u
        r.ls = stage_point(lam, d.lks, LSTAGE_C) if c.op == "vjp_stage" else lam
        r.lamJ, r.dp = O.fk_vjp(c.spec(), p, D, dx, r.y, r.ls)
        _, r.s_lamJ, r.s_dp = scales(c, p, r.y, r.ls)
        if c.op == "vjp_stage":
            r.err, b = err_norm(STAGE_EC, d.lks, r.lamJ, lam, r.ls)
            r.err_bound = b(1e-13 * r.s_lamJ)
    return r


# ---- wrong restatements, applied to the oracle's output in numpy ----------------------------------------------------
def _lap_co(c):
    D, dx = c.D_dx
    return N.fk_coeffs(D, dx)[1]


def mutate(c, d, r, which):
    """The reference r with one thing wrong; returns a dict of the outputs the mutation changes.  The stencil
    mutations act on the field the Laplacian is taken of (the stage point for "stage", λs for the VJP forms)."""
    co = _lap_co(c)
    out = "du" if c.op in ("rhs", "stage") else "lamJ"
    v = {"rhs": d.u, "stage": getattr(r, "y", None), "vjp": d.lam, "vjp_stage": getattr(r, "ls", None)}[c.op]
    ref = getattr(r, out)
    nx, B = c.nx, ref.shape[0]
    if which == "wrap_same_segment":      # lane 0 / lane 63 take their outer neighbour from their own segment
        g = ref.copy()
        for k in range(NP_OF[nx]):
            i0, i1 = 128 * k, 128 * k + 127
            g[:, i0] += co * (v[:, i1] - v[:, (i0 - 1) % nx])
            g[:, i1] += co * (v[:, i0] - v[:, (i1 + 1) % nx])
        return {out: g}
    if which == "swap_um_up":             # lane 0's left neighbour is its right one, lane 63's right its left one
        g = ref.copy()
        for k in range(NP_OF[nx]):
            i0, i1 = 128 * k, 128 * k + 127
            g[:, i0] += co * (v[:, i0 + 2] - v[:, (i0 - 1) % nx])
            g[:, i1] += co * (v[:, i1 - 2] - v[:, (i1 + 1) % nx])
        return {out: g}
    if which == "stale_last_row":         # the last row of every block's range keeps a stale (zero) buffer
        g = ref.copy()
        blk = c.block_of()
        last = np.array([np.max(np.nonzero(blk == b)[0]) for b in np.unique(blk)])
        g[last] = 0.0
        return {out: g}
    if which == "slipped_pipeline":       # a row holds the result of its wave's next trip's row
        g = ref.copy()
        blk, trip = c.block_of(), c.trip_of()
        stride = WPB if c.launch.chunk else WPB * c.launch.grid
        for b in range(B):
            n = b + stride
            if n < B and blk[n] == blk[b] and trip[n] == trip[b] + 1:
                g[b] = ref[n]
        return {out: g}
    if which == "generic_small":          # nx = 2 as an interior row: the corner counted twice
        D, dx = c.D_dx
        cd, co2 = N.fk_coeffs(D, dx)
        return {out: ref - FC.lap_apply(v, cd, co2) + FC.lap_apply(v, cd, co2, "generic_small")}
    if which == "dp_less_a_block":        # the last block's slab row never reaches dp
        blk = c.block_of()
        dead = blk == np.max(blk)
        D, dx = c.D_dx
        _, part = O.fk_vjp(c.spec(), d.p, D, dx, r.y[dead], r.ls[dead])
        return {"dp": r.dp - part}
    if which == "stage_less_last_k":      # y = u + Σ_{j < last} c_j k_j
        D, dx = c.D_dx
        y = stage_point(d.u, d.ks[:-1], STAGE_C[:-1])
        if c.op == "stage":
            return {"du": O.fk_rhs(c.spec(), d.p, D, dx, y)}
        g, dp = O.fk_vjp(c.spec(), d.p, D, dx, y, r.ls)
        return {"lamJ": g, "dp": dp}
    if which == "err_scaled_by_lam":      # sk = abstol + reltol·|lam|, without the max against |λs|
        return {"err": err_norm(STAGE_EC, d.lks, r.lamJ, d.lam, d.lam)[0]}
    raise KeyError(which)


def _wave(c):
    return c.launch.family in ("wave_rhs", "stage", "vjp", "vjp_stage")


def _second_trip(c):
    return _wave(c) and int(np.max(c.trip_of())) >= 1


# name: (the records of its group, the condition under which it is visible, stated)
MUTATIONS = {
    # visible when D != 0 and the two neighbours differ (every row drawn independently)
    "wrap_same_segment": lambda c: _wave(c) and c.nx >= 256 and c.diff == "Ddx2",
    "swap_um_up": lambda c: _wave(c) and c.diff == "Ddx2",
    # visible when the row's result is not zero
    "stale_last_row": lambda c: _wave(c),
    # visible when the rows differ
    "slipped_pipeline": _second_trip,
    "generic_small": lambda c: c.nx == 2 and c.diff == "Ddx2" and c.B != "big",
    # visible when the last block's rows have λ != 0
    "dp_less_a_block": lambda c: c.op in ("vjp", "vjp_stage") and c.launch.grid >= 2,
    # visible when c_last·k_last != 0
    "stage_less_last_k": lambda c: c.op in ("stage", "vjp_stage"),
    # visible when |λs| > |lam| at points that carry weight in the norm
    "err_scaled_by_lam": lambda c: c.op == "vjp_stage",
}
# where a mutation cannot occur it must change nothing (the CPU test holds it to exactly the reference there)
CANNOT = {
    "wrap_same_segment": lambda c: _wave(c) and c.diff == "D0",
    "swap_um_up": lambda c: _wave(c) and c.diff == "D0",
    "slipped_pipeline": lambda c: _wave(c) and not _second_trip(c),
}
