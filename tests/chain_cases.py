"""The cases the parity matrix of the small-chain kernels shares (test_chain_cases_cpu.py, test_gpu_chain_matrix.py):
the table of records, the rung and the launchers each record is meant to reach (kan_col.hip: kd_chain_col_kernel
behind launch_kd_chain_col, kd_chain_vjp_stage_kernel + chain_vjp_finish_kernel behind launch_kd_chain_vjp_stage,
kd_chain_step_kernel, kd_chain_vjp_step_kernel; the predicates of kan_chain_plan.hpp), its seeded inputs, and the
numpy statement of the chain in the kernels' order with its wrong restatements.  No tests live here.

The pass criterion everywhere is gpu_util.assert_close(got, ref, scale, gpu_util.RTOL[dtype]) under the scales of
layer_cases.py as they stand (error_scale / chain_error_scale against the oracle, composition_error_scale against the
layer calls on the same device, layer_error_scale for a single layer call).

What a record states by hand, per dtype: its rung (LV, TanhRec, RecCorr, Rec, Direct; None where the layers do not
share one), whether the one-launch forward kernel serves rhs, whether the one-launch pullback kernel serves vjp.
served_restated restates the launch rules from the code and can drift from it: test_chain_cases_cpu.py holds the
hand-stated classes against kan_chain_plan.hpp itself (tests/host/chain_record_probe.cpp) and against this
restatement, and the GPU matrix reaches a launcher only through the library's own rule and reads back which one ran
(KANODE_OPT_LAST_EVAL).

Sizes and caps, from the code: sizeof(LayerConst) = 1248; a layer is of the column class while P_layer <= 2048 (and
O <= 16, (G·I + O + I)·65·esize <= 150 KiB); the forward kernel stages nl·1248 + P·esize <= 49,152 B and takes
2 <= nl <= 8 layers and K <= 32,768 columns; the pullback kernel stages nl·1248 + P·esize·(1 + 4) <= 61,440 B, takes
1 <= nl <= 4 layers and needs N_in == N_out; its blocks hold 4 columns, one block writes dp itself (K <= 4), more
blocks write slab rows that chain_vjp_finish_kernel sums, and the grid is capped at 1024 blocks, so column 4096 is the
first of the loop's second trip.  The forward kernel's blocks hold 16 columns: one block sums a stage's error itself
(K <= 16), more go through the error slab."""
from __future__ import annotations

import zlib
from dataclasses import dataclass

import numpy as np

import fk_cases as FK
import layer_cases as LC
from oracle import kanode_np as N
from oracle import oracle as O

LV, TANH_REC, REC_CORR, REC, DIRECT = "LV", "TanhRec", "RecCorr", "Rec", "Direct"
RUNGS = (LV, TANH_REC, REC_CORR, REC, DIRECT)
RUNG_ID = {LV: 0, TANH_REC: 1, REC_CORR: 2, REC: 3, DIRECT: 4}                 # kan_chain_plan.hpp ChainRung
NORM_ID = {"tanh_fast": 0, "tanh": 1, "softsign": 2, "sigmoid": 3, "sigmoid_fast": 4, "identity": 5}   # kan_device.hpp
PATH_ID = {FK.DIRECT: 0, FK.REC: 1, FK.REC_CORR: 2}                            # kan_device.hpp Path
LC_BYTES, COL_P, FWD_BUDGET, VJP_BUDGET, FWD_LAYERS, VJP_LAYERS = 1248, 2048, 49152, 61440, 8, 4
CHAIN_DIM, FWD_MAX_K, VJP_GROUPS, VJP_GRID_CAP, FWD_COLS = 16, 32768, 4, 1024, 16

# the launcher an evaluation call reports (kanode_eval_path, include/kanode.h)
EVAL_CHAIN_KERNEL, EVAL_CHAIN_STEP, EVAL_CHAIN_ADJ_STEP, EVAL_PER_LAYER = 1, 2, 3, 4


@dataclass(frozen=True)
class Cls:
    rung: str | None    # None: the layers do not share a normalizer / path, no rung is asked for
    fwd: bool           # kd_chain_col_kernel serves rhs
    vjp: bool           # kd_chain_vjp_stage_kernel serves vjp


def _c(rung, fwd, vjp):
    return Cls(rung, bool(fwd), bool(vjp))


@dataclass(frozen=True)
class Row:
    name: str
    widths: tuple
    G: object                       # one grid length, or one per layer
    norm: object                    # one normalizer, or one per layer
    f64: Cls
    f32: Cls
    batches: tuple = (1, 5, 17)
    basis: str = "rbf"
    lims: tuple = (-1.0, 1.0)
    den: float = None
    quirk: bool = True
    base: str = "all"               # "all" / "none" / "first"
    fwd_only: bool = False          # the large batches: the pullback is not run
    notes: tuple = ()               # the launch-shape claims the row is there for, beyond what its classes give

    @property
    def n_layers(self):
        return len(self.widths) - 1

    def per_layer(self, v):
        return tuple(v) if isinstance(v, (tuple, list)) else (v,) * self.n_layers


FULL_B = (1, 4, 5, 16, 17)
TF, SS = "tanh_fast", "softsign"
_BOTH = dict(f64=_c(TANH_REC, 1, 1), f32=_c(TANH_REC, 1, 1))

ROWS = [
    # ---- rungs ---------------------------------------------------------------------------------------------------
    # the Lotka-Volterra shape: ChainShapeLV, layer 0 output-major
    Row("lv", (2, 10, 2), 5, TF, _c(LV, 1, 1), _c(LV, 1, 1), FULL_B + (4099,)),
    Row("lv_nobase", (2, 10, 2), 5, TF, _c(LV, 1, 1), _c(LV, 1, 1), base="none"),
    Row("lv_base0", (2, 10, 2), 5, TF, _c(LV, 1, 1), _c(LV, 1, 1), base="first"),
    # K = 32,768 is the forward kernel's last batch; 32,769 runs layer by layer (forward only)
    Row("lv_k32768", (2, 10, 2), 5, TF, _c(LV, 1, 1), _c(LV, 1, 1), (32768,), fwd_only=True, notes=("k_edge_in",)),
    Row("lv_k32769", (2, 10, 2), 5, TF, _c(LV, 0, 1), _c(LV, 0, 1), (32769,), fwd_only=True, notes=("k_edge_out",)),
    # either side of chain_is_lv: the LV widths with another G
    Row("lvw_g53", (2, 10, 2), (5, 3), TF, batches=FULL_B + (4099,), **_BOTH),
    Row("lvw_g3", (2, 10, 2), 3, TF, **_BOTH),
    Row("lv_t", (10, 2, 10), 5, TF, **_BOTH),
    Row("ss_g7", (3, 6, 3), 7, SS, _c(REC_CORR, 1, 1), _c(REC_CORR, 1, 1), FULL_B + (4099,)),
    Row("ss_g7_small", (3, 4, 3), 7, SS, _c(REC_CORR, 1, 1), _c(REC_CORR, 1, 1)),      # P = 192 (ADJ_STEP below)
    Row("tanh_g10", (3, 6, 3), 10, "tanh", _c(REC_CORR, 1, 1), _c(DIRECT, 1, 1), FULL_B + (4099,)),
    Row("ss_g5", (3, 6, 3), 5, SS, _c(REC, 1, 1), _c(REC, 1, 1), FULL_B + (4099,)),
    Row("ss_g5_nobase", (3, 6, 3), 5, SS, _c(REC, 1, 1), _c(REC, 1, 1), base="none"),
    Row("ss_g5_base0", (3, 6, 3), 5, SS, _c(REC, 1, 1), _c(REC, 1, 1), base="first"),
    Row("sig01_g5", (3, 5, 3), 5, "sigmoid", _c(REC, 1, 1), _c(REC, 1, 1), lims=(0.0, 1.0)),
    Row("tanh_g3", (3, 4, 3), 3, "tanh", _c(REC, 1, 1), _c(REC, 1, 1)),
    Row("ss_den04", (3, 6, 3), 5, SS, _c(REC, 1, 1), _c(REC, 1, 1), den=0.4),
    Row("tanh_rswaf", (3, 6, 3), 5, "tanh", _c(DIRECT, 1, 1), _c(DIRECT, 1, 1), FULL_B + (4099,), basis="rswaf"),
    Row("ss_iqf_quirk", (3, 6, 3), 5, SS, _c(DIRECT, 1, 1), _c(DIRECT, 1, 1), basis="iqf"),
    Row("ss_iqf_exact", (3, 6, 3), 5, SS, _c(DIRECT, 1, 1), _c(DIRECT, 1, 1), basis="iqf", quirk=False),
    Row("ident_nobase", (3, 4, 3), 5, "identity", _c(DIRECT, 1, 1), _c(DIRECT, 1, 1), base="none"),
    # layers that differ in G within one path (softsign G = 3 and 5 are both REC)
    Row("mix_g35", (3, 8, 3), (3, 5), SS, _c(REC, 1, 1), _c(REC, 1, 1)),
    # ---- widths ----------------------------------------------------------------------------------------------------
    Row("w1_1_1", (1, 1, 1), 5, TF, **_BOTH),
    Row("w1_16_1", (1, 16, 1), 5, TF, **_BOTH),
    # P = 768: the pullback kernel at kChainDim in both dtypes (2496 + 768·8·5 = 33,216 B)
    Row("w16_4_16", (16, 4, 16), 5, TF, **_BOTH),
    Row("w4_16_4", (4, 16, 4), 5, TF, **_BOTH),
    # P = 1024: full width in both layers, fp64 pullback included (2496 + 1024·8·5 = 43,456 B)
    Row("w16x3_g2_nobase", (16, 16, 16), 2, TF, base="none", **_BOTH),
    # P = 1440: 2496 + 1440·8·5 = 60,096 B fits
    Row("w15_16_15_g2", (15, 16, 15), 2, TF, notes=("vjp_budget_in:f64",), **_BOTH),
    # P = 2880: the pullback budget's two sides in one shape: fp64 2496 + 115,200 B, fp32 2496 + 57,600 = 60,096 B
    Row("w15_16_15_g5", (15, 16, 15), 5, TF, _c(TANH_REC, 1, 0), _c(TANH_REC, 1, 1),
        notes=("vjp_budget_out:f64", "vjp_budget_in:f32")),
    # P = 3072 (layer_cases' edge record): forward only; fp32 2496 + 61,440 B is over by the constants alone
    Row("w16x3_g5", (16, 16, 16), 5, TF, _c(TANH_REC, 1, 0), _c(TANH_REC, 1, 0),
        notes=("vjp_budget_out:f64", "vjp_budget_out:f32")),
    # ... without the base term P = 2560: fp32 2496 + 51,200 B fits, fp64 2496 + 102,400 B does not
    Row("w16x3_g5_nobase", (16, 16, 16), 5, TF, _c(TANH_REC, 1, 0), _c(TANH_REC, 1, 1), base="none",
        notes=("vjp_budget_out:f64", "vjp_budget_in:f32")),
    # ---- depth -----------------------------------------------------------------------------------------------------
    # one layer: never the chain forward (n_layers > 1); the pullback kernel when N_in == N_out
    Row("d1", (3, 3), 5, TF, _c(TANH_REC, 0, 1), _c(TANH_REC, 0, 1)),
    Row("d1_ss7", (3, 3), 7, SS, _c(REC_CORR, 0, 1), _c(REC_CORR, 0, 1)),
    Row("d1_ne", (2, 3), 5, TF, _c(TANH_REC, 0, 0), _c(TANH_REC, 0, 0)),
    Row("d3", (3, 6, 5, 3), 5, TF, **_BOTH),
    Row("d3_ss7", (3, 6, 5, 3), 7, SS, _c(REC_CORR, 1, 1), _c(REC_CORR, 1, 1)),
    Row("d4", (3, 5, 4, 5, 3), 5, TF, **_BOTH),
    Row("d4_ss5", (3, 5, 4, 5, 3), 5, SS, _c(REC, 1, 1), _c(REC, 1, 1)),
    Row("d4_rswaf", (3, 5, 4, 5, 3), 5, "tanh", _c(DIRECT, 1, 1), _c(DIRECT, 1, 1), basis="rswaf"),
    # past kChainMaxLayers: the forward kernel still, the pullback layer by layer
    Row("d5", (3, 4, 5, 4, 5, 3), 5, TF, _c(TANH_REC, 1, 0), _c(TANH_REC, 1, 0)),
    Row("d5_ss7", (3, 4, 5, 4, 5, 3), 7, SS, _c(REC_CORR, 1, 0), _c(REC_CORR, 1, 0)),
    Row("d8", (3, 4, 3, 4, 3, 4, 3, 4, 3), 3, TF, _c(TANH_REC, 1, 0), _c(TANH_REC, 1, 0)),
    # ---- N_in != N_out ---------------------------------------------------------------------------------------------
    Row("ne_2_10_3", (2, 10, 3), 5, TF, _c(TANH_REC, 1, 0), _c(TANH_REC, 1, 0)),
    # ---- the 48 KiB parameter budget ---------------------------------------------------------------------------------
    # P = 3·2048 = 6144: fp64 49,152 + 3,744 B is over, fp32 24,576 + 3,744 B fits
    Row("b16x4_g7", (16, 16, 16, 16), 7, SS, _c(REC_CORR, 0, 0), _c(REC_CORR, 1, 0),
        notes=("fwd_budget_out:f64", "fwd_budget_in:f32")),
    # P = 3·1792 = 5376: fp64 43,008 + 3,744 = 46,752 B fits
    Row("b16x4_g6", (16, 16, 16, 16), 6, SS, _c(REC_CORR, 1, 0), _c(REC_CORR, 1, 0),
        notes=("fwd_budget_in:f64", "fwd_budget_in:f32")),
    # six such layers, P = 12,288: fp32 49,152 + 7,488 B is over as well (five would fit: 40,960 + 6,240 B)
    Row("b16x6_g7", (16,) * 7, 7, SS, _c(REC_CORR, 0, 0), _c(REC_CORR, 0, 0), (1, 5),
        notes=("fwd_budget_out:f64", "fwd_budget_out:f32")),
    # ---- refused on purpose: per layer ----------------------------------------------------------------------------
    Row("r_norms", (3, 6, 5, 3), 4, (TF, SS, TF), _c(None, 0, 0), _c(None, 0, 0)),
    Row("r_sigmoids", (3, 5, 3), 5, ("sigmoid", "sigmoid_fast"), _c(None, 0, 0), _c(None, 0, 0), lims=(0.0, 1.0)),
    Row("r_g57", (3, 6, 3), (5, 7), SS, _c(None, 0, 0), _c(None, 0, 0)),
]
BY_NAME = {r.name: r for r in ROWS}
PLANT_FROM_B = 16     # a record has room for the planted inputs from this batch on (module docstring of Case.data)


@dataclass(frozen=True)
class Case:
    row: Row
    dtype: str      # "f64" / "f32"
    B: int

    @property
    def id(self):
        return f"{self.row.name}-{self.dtype}-B{self.B}"

    @property
    def seed(self):
        return zlib.crc32(self.id.encode())

    @property
    def n_layers(self):
        return self.row.n_layers

    @property
    def esize(self):
        return 8 if self.dtype == "f64" else 4

    @property
    def cls(self):
        """The classes this record is meant to reach (stated by hand in ROWS)."""
        return getattr(self.row, self.dtype)

    @property
    def base(self):
        return [self.row.base == "all" or (self.row.base == "first" and l == 0) for l in range(self.n_layers)]

    @property
    def P(self):
        return sum(s.param_length() for s in self.specs())

    @property
    def square(self):
        return self.row.widths[0] == self.row.widths[-1]

    @property
    def rhs_path(self):
        """What KANODE_OPT_LAST_EVAL reads after rhs / after vjp with λᵀJ."""
        return EVAL_CHAIN_KERNEL if self.cls.fwd else EVAL_PER_LAYER

    @property
    def vjp_path(self):
        return EVAL_CHAIN_KERNEL if self.cls.vjp else EVAL_PER_LAYER

    @property
    def rhs_stage_path(self):
        """... after rhs_stage (square records): stage_t asks the forward kernel for a single layer too."""
        served = self.cls.fwd or (self.n_layers == 1 and self.cls.rung is not None)
        return EVAL_CHAIN_KERNEL if served else EVAL_PER_LAYER

    @property
    def claims(self):
        """What of REQUIRED this record covers, from the hand-stated classes and the batch."""
        c = self.cls
        out = {("serve", c.fwd, c.vjp)}
        if c.rung is not None and (c.fwd or c.vjp):
            out.add(("rung", c.rung))
        if c.fwd:
            out.add("fwd_one_block" if self.B <= FWD_COLS else "fwd_error_slab")
        if c.vjp and not self.row.fwd_only:
            out.add("vjp_single_block" if self.B <= VJP_GROUPS else "vjp_finish_launch")
            if self.B > VJP_GROUPS * VJP_GRID_CAP:
                out.add("vjp_second_trip")
        for n in self.row.notes:
            what, _, dt = n.partition(":")
            if not dt or dt == self.dtype:
                out.add(what)
        return out

    def specs(self):
        r = self.row
        G, norm, base = r.per_layer(r.G), r.per_layer(r.norm), self.base
        return [O.LayerSpec(r.widths[l], r.widths[l + 1], G[l], norm[l], r.basis, base[l], r.lims, r.den, r.quirk)
                for l in range(self.n_layers)]

    def np_dtype(self):
        return np.float64 if self.dtype == "f64" else np.float32

    def data(self):
        """(p, u, ȳ) in float64, as layer_cases.Case.data: Glorot-uniform parameters (no W block without the base
        activation), inputs uniform inside the grid limits, ȳ standard normal; an fp32 record's values are rounded to
        fp32 first.  A record of B >= 16 columns has room for fk_cases' planted inputs beside random ones: exactly 0,
        +1e4 and -1e4 at seeded places of u (the normalizer saturates, swish is x or 0).  The smaller batches stay
        unplanted on purpose: a planted 1e4 raises the scales' floor (1e-3 of the largest entry) for every other
        column of the record."""
        rng = np.random.default_rng(self.seed)
        parts = []
        for s in self.specs():
            lim = np.sqrt(6.0 / (s.out_dims + s.grid_len * s.in_dims))
            parts.append(rng.uniform(-lim, lim, s.out_dims * s.grid_len * s.in_dims))
            if s.use_base_act:
                lim = np.sqrt(6.0 / (s.out_dims + s.in_dims))
                parts.append(rng.uniform(-lim, lim, s.out_dims * s.in_dims))
        lo, hi = self.row.lims
        p = np.concatenate(parts)
        u = rng.uniform(lo, hi, (self.B, self.row.widths[0]))
        yb = rng.normal(size=(self.B, self.row.widths[-1]))
        if self.B >= PLANT_FROM_B:
            u.reshape(-1)[rng.choice(u.size, 3, replace=False)] = [0.0, 1e4, -1e4]
        dt = self.np_dtype()
        return tuple(a.astype(dt).astype(np.float64) for a in (p, u, yb))


def _cases():
    return [Case(r, dt, B) for r in ROWS for dt in ("f64", "f32") for B in r.batches]


CASES = _cases()

# what the table has to reach, per dtype (test_chain_cases_cpu.py: each claimed by a record whose classes the header
# confirms): every rung, the four combinations of the two launchers, the pullback's one block / finish launch /
# second trip, the forward's one block / error slab, both sides of the two LDS budgets and of the batch edge
REQUIRED = ({("rung", r) for r in RUNGS} | {("serve", f, v) for f in (True, False) for v in (True, False)}
            | {"vjp_single_block", "vjp_finish_launch", "vjp_second_trip", "fwd_one_block", "fwd_error_slab",
               "fwd_budget_in", "fwd_budget_out", "vjp_budget_in", "vjp_budget_out", "k_edge_in", "k_edge_out"})
# the second trip of the pullback's column loop: one record per rung and dtype
SECOND_TRIP_B = 4099

# The fused steps (kd_chain_step_kernel, kd_chain_vjp_step_kernel), at B = 17 (past the one-workgroup solve's 16):
# one generic two-layer row per rung plus LV.  row: whether the fused ADJOINT step serves it, (fp64, fp32), stated by
# hand.  It keeps seven gradient rows per column group in LDS (chain_vjp_step_supported):
# nl·1248 + P·esize·(1 + 7·4) <= 65,536 B, i.e. P <= 271 in fp64 and P <= 543 in fp32 for two layers.  Where it does
# not fit the integrator runs the one-launch adjoint STAGE kernel six times per step, again without an error.  The
# forward step has the forward kernel's conditions and serves every row here.
#   lv 240: 2496 + 55,680;  lvw_g53 200: 2496 + 46,400;  ss_g7_small 192: 2496 + 44,544;  ss_g5 216: 2496 + 50,112;
#   tanh_rswaf 216;  ss_g7 288: 2496 + 66,816 (over in fp64; fp32 2496 + 33,408);  tanh_g10 396: 2496 + 91,872 (over
#   in fp64; fp32 2496 + 45,936)
ADJ_STEP = {"lv": (True, True), "lvw_g53": (True, True), "ss_g7_small": (True, True), "ss_g5": (True, True),
            "tanh_rswaf": (True, True), "ss_g7": (False, True), "tanh_g10": (False, True)}
STEP_B = 17


# ---- the launch rules, restated ---------------------------------------------------------------------------------
def layer_paths(case):
    """The basis path of every layer: fk_cases.fk_path of the layer's spec (make_layer_const)."""
    return [FK.fk_path(case.dtype, s) for s in case.specs()]


def rung_restated(case):
    """chain_rung of kan_chain_plan.hpp on layer 0 (None where the layers differ in normalizer or path)."""
    specs, paths = case.specs(), layer_paths(case)
    if any(s.normalizer != specs[0].normalizer for s in specs) or any(q != paths[0] for q in paths):
        return None
    r = case.row
    if specs[0].normalizer == "tanh_fast" and paths[0] == FK.REC:
        lv = r.widths == (2, 10, 2) and r.per_layer(r.G) == (5, 5)
        return LV if lv else TANH_REC
    return {FK.REC_CORR: REC_CORR, FK.REC: REC, FK.DIRECT: DIRECT}[paths[0]]


def served_restated(case):
    """(forward kernel serves rhs, pullback kernel serves vjp): rhs_t / vjp_t of kanode_eval.cpp and the two launchers
    of kan_col.hip, restated (module docstring)."""
    specs, nl = case.specs(), case.n_layers
    all_col = all(LC.kernel_class(s.in_dims, s.out_dims, s.grid_len, s.use_base_act, case.esize) == LC.COL
                  for s in specs)
    small = all(max(s.in_dims, s.out_dims) <= CHAIN_DIM for s in specs) and rung_restated(case) is not None
    fwd = (all_col and small and 2 <= nl <= FWD_LAYERS and case.B <= FWD_MAX_K
           and nl * LC_BYTES + case.P * case.esize <= FWD_BUDGET)
    vjp = (all_col and small and 1 <= nl <= VJP_LAYERS and case.square
           and nl * LC_BYTES + case.P * case.esize * (1 + VJP_GROUPS) <= VJP_BUDGET)
    return fwd, vjp


def probe_line(case):
    """The record as tests/host/chain_record_probe.cpp reads it: id, esize, P, B, nl, then I O G norm path per layer."""
    f = [case.id, case.esize, case.P, case.B, case.n_layers]
    for s, q in zip(case.specs(), layer_paths(case)):
        f += [s.in_dims, s.out_dims, s.grid_len, NORM_ID[s.normalizer], PATH_ID[q]]
    return " ".join(str(v) for v in f)


# ---- the chain in the kernels' order, in numpy --------------------------------------------------------------------
def _fma(f, a, b, c):
    """fma in dtype f: exact product and one rounding in fp32 (the product of two fp32 values is exact in float64);
    plain a·b + c in float64."""
    if f == np.float32:
        return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f)
    return a * b + c


def _row16_sum(v, drop_lane15=False):
    """The 16-lane butterfly sum over axis 1 of v (K, I <= 16, ...): every lane takes part, the idle ones with 0."""
    pad = np.zeros((v.shape[0], CHAIN_DIM) + v.shape[2:], v.dtype)
    pad[:, :v.shape[1]] = v
    if drop_lane15:
        pad[:, 15] = 0
    for s in (1, 2, 4, 8):
        pad = pad + pad[:, np.arange(CHAIN_DIM) ^ s]
    return pad[:, 0]


class _KLayer:
    """One layer as a column group of kd_chain_col_kernel / chain_pullback evaluates it, in dtype f: lane i forms its
    partial sums over g by fma, a 16-lane butterfly sums the lanes, the base term is summed apart and added last.  The
    basis is evaluated directly (the statement of what is computed; the recurrence paths compute the same values)."""

    def __init__(self, spec, f, exact_knots=False):
        self.L = LC.np_layers([spec])[0]
        self.f = f
        L = self.L
        self.grid = L.grid.astype(f)
        if exact_knots:   # float64-exact knots lo + j·(hi - lo)/(G - 1) in place of the Float32 LinRange knots
            lo, hi = float(np.float32(spec.grid_lims[0])), float(np.float32(spec.grid_lims[1]))
            self.grid = (lo + np.arange(L.G, dtype=np.float64) * (hi - lo) / (L.G - 1)).astype(f)
        self.invh = f(L.invh)

    def basis(self, x):
        L, f = self.L, self.f
        n = N.NORMS[L.normalizer](x).astype(f)
        z = (n[:, :, None] - self.grid[None, None, :]) * self.invh
        if L.basis == "rbf":
            phi = np.exp(-(z * z))
        elif L.basis == "rswaf":
            phi = 1 - np.tanh(z) ** 2
        else:
            phi = 1 / (1 + z * z)
        return n, z.astype(f), phi.astype(f)

    def split(self, pl, no_base=False):
        L = self.L
        C, W = L.split(pl.astype(self.f))
        Cr = C.reshape(L.O, L.I, L.G)
        if W is not None and no_base:
            W = np.zeros_like(W)
        return Cr, W

    def fwd(self, pl, x, drop_lane15=False, no_base=False):
        L, f = self.L, self.f
        Cr, W = self.split(pl, no_base)
        _, _, phi = self.basis(x)
        acc = np.zeros((x.shape[0], L.I, L.O), f)
        for g in range(L.G):
            acc = _fma(f, Cr[:, :, g].T[None], phi[:, :, g, None], acc)
        y = _row16_sum(acc, drop_lane15)
        if L.use_base_act:
            sw = N.swish(x).astype(f)
            y = y + _row16_sum(W.T[None] * sw[:, :, None], drop_lane15)
        return y.astype(f)

    def pull(self, pl, x, yb, no_base=False):
        """(x̄ (K, I), the columns' contributions to p̄ (K, P_layer)) in chain_pullback's order."""
        L, f = self.L, self.f
        Cr, W = self.split(pl, no_base)
        n, z, phi = self.basis(x)
        K = x.shape[0]
        bb = np.zeros((K, L.I, L.G), f)
        for o in range(L.O):
            bb = _fma(f, Cr[o][None], yb[:, o, None, None], bb)
        if L.basis == "rbf":
            zb = f(-2) * z * phi * bb
        elif L.basis == "rswaf":
            zb = f(-2) * np.tanh(z) * phi * bb
        else:
            zb = f(-2) * z * phi * bb if L.iqf_reference_quirk else f(-2) * z * phi * phi * bb
        nbar = np.zeros((K, L.I), f)
        for g in range(L.G):
            nbar = nbar + zb[:, :, g].astype(f) * self.invh
        xb = nbar * N.dnorm(L.normalizer, x, n).astype(f)
        parts = [(phi[:, :, :, None] * yb[:, None, None, :]).reshape(K, -1)]          # (i, g, o), o fastest
        if L.use_base_act:
            sw, dsw = N.swish(x).astype(f), N.dswish(x).astype(f)
            sb = np.zeros((K, L.I), f)
            for o in range(L.O):
                sb = _fma(f, W[o][None], yb[:, o, None], sb)
            xb = xb + sb * dsw
            dW = sw[:, :, None] * yb[:, None, :]
            parts.append((np.zeros_like(dW) if no_base else dW).reshape(K, -1))
        return xb.astype(f), np.concatenate(parts, axis=1).astype(f)


MUTATION_DOC = {
    "skip_last_out": "output slot O - 1 of the last layer is not summed (y of that slot stays 0)",
    "drop_lane15": "lane 15 is left out of the row sums of a 16-wide layer input",
    "swap_outmajor": "the two inputs of the output-major layer (LV layer 0) are swapped",
    "no_base_l1": "the base term is missing from every layer l >= 1",
    "exact_knots": "float64-exact knots in place of the Float32 LinRange knots (what PATH_REC_CORR corrects for)",
    "first_group_dp": "dp is taken from the first column group of each block only",
    "first_trip": "the columns past the first trip of the pullback's loop are dropped",
    "skip_layer4": "the fourth layer is skipped (its input passed on, cut or zero-filled to its output width)",
    "dp_assign": "dp is assigned where it is to accumulate onto the caller's dp",
}


def _resize(a, n):
    out = np.zeros((a.shape[0], n), a.dtype)
    m = min(n, a.shape[1])
    out[:, :m] = a[:, :m]
    return out


def np_chain(case, p, u, yb, f=np.float64, mut=None, dp0=None):
    """(y, x̄, p̄) of the chain as the small-chain kernels state it, in dtype f (np.float32: the fp32 statement the bars
    have to hold; np.float64 with mut: one wrong restatement of MUTATION_DOC).  The columns' p̄ contributions are
    summed as kd_chain_vjp_stage_kernel and chain_vjp_finish_kernel do: per column group over the loop's trips, the
    four groups of a block, then the blocks.  dp0: p̄ accumulates onto it."""
    assert mut is None or mut in MUTATION_DOC
    specs = case.specs()
    Ls = [_KLayer(s, f, exact_knots=mut == "exact_knots") for s in specs]
    offs = np.cumsum([0] + [s.param_length() for s in specs])
    p, u, yb = p.astype(f), u.astype(f), yb.astype(f)
    K = u.shape[0]

    def layer_fwd(l, x):
        if mut == "skip_layer4" and l == 3:
            return _resize(x, specs[l].out_dims)
        if mut == "swap_outmajor" and l == 0:
            x = x[:, ::-1]
        return Ls[l].fwd(p[offs[l]:offs[l + 1]], x, drop_lane15=mut == "drop_lane15" and specs[l].in_dims == 16,
                         no_base=mut == "no_base_l1" and l >= 1)

    acts = [u]
    for l in range(len(specs)):
        acts.append(layer_fwd(l, acts[-1]))
    y = acts[-1].copy()
    if mut == "skip_last_out":
        y[:, -1] = 0
    g = yb
    contrib = [None] * len(specs)
    for l in range(len(specs) - 1, -1, -1):
        if mut == "skip_layer4" and l == 3:
            contrib[l] = np.zeros((K, specs[l].param_length()), f)
            g = _resize(g, specs[l].in_dims)
            continue
        x = acts[l][:, ::-1] if mut == "swap_outmajor" and l == 0 else acts[l]
        g, contrib[l] = Ls[l].pull(p[offs[l]:offs[l + 1]], x, g, no_base=mut == "no_base_l1" and l >= 1)
    xb = g
    rows = np.concatenate(contrib, axis=1)                    # (K, P)
    grid = min((K + VJP_GROUPS - 1) // VJP_GROUPS, VJP_GRID_CAP)
    per_trip = grid * VJP_GROUPS
    trips = (K + per_trip - 1) // per_trip
    if mut == "first_trip":
        xb = xb.copy()
        xb[per_trip:] = 0
        trips = 1
    padded = np.zeros((trips * per_trip, rows.shape[1]), f)
    m = min(K, trips * per_trip)
    padded[:m] = rows[:m]
    padded = padded.reshape(trips, grid, VJP_GROUPS, -1)
    grp = padded[0]
    for t in range(1, trips):
        grp = grp + padded[t]
    blk = grp[:, 0]
    if mut != "first_group_dp":
        for q in range(1, VJP_GROUPS):
            blk = blk + grp[:, q]
    pb = blk[0] if grid == 1 else np.sum(blk, axis=0, dtype=f)
    if dp0 is not None and mut != "dp_assign":
        pb = dp0.astype(f) + pb
    return y, xb, pb.astype(f)


# name: the records of the mutation's group (the classes are the hand-stated ones)
MUTATIONS = {
    "skip_last_out": lambda c: True,
    "drop_lane15": lambda c: 16 in c.row.widths[:-1],
    "swap_outmajor": lambda c: c.cls.rung == LV,
    "no_base_l1": lambda c: any(c.base[1:]),
    # fp32 cannot see it by construction of the bar: the knots move by an fp32 rounding of the knot, and the scale's
    # a_err term allows exactly one such rounding of n - knot (layer_cases: invh·(n_err + |knot|)); as in the other two
    # matrices the restatement is asked of the fp64 records
    "exact_knots": lambda c: c.dtype == "f64" and c.cls.rung == REC_CORR,
    "first_group_dp": lambda c: c.B >= 2 and not c.row.fwd_only,
    "first_trip": lambda c: c.B == SECOND_TRIP_B,
    "skip_layer4": lambda c: c.n_layers >= 4,
    "dp_assign": lambda c: not c.row.fwd_only,
}
