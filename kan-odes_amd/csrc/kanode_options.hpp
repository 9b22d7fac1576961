// kanode_options.hpp — the handle's evaluation-strategy options (include/kanode.h, kanode_set_option): the fields,
// and ONE table that states each option's id, name, kind, upper bound and field.  kanode_set_option and
// kanode_get_option are options_set / options_get over it.  Host-only and HIP-free (kanode.h and the standard
// library), so tests/host/options_test.cpp checks it as a stand-alone program.
#pragma once
#include <stdint.h>

#include <string>

#include "kanode.h"

// (private to the library: nothing here enters its dynamic symbol table)
#pragma GCC visibility push(hidden)

#ifndef KAN_SLAB_BLOCKS
#define KAN_SLAB_BLOCKS 4096
#endif
constexpr int kSlabBlocks = KAN_SLAB_BLOCKS;   // grid cap of the VJP kernels = slab rows

// Read when a call is issued, never from the environment per launch.  Flags are 0 / 1.
struct HandleOptions {
    int pp_on = 0;   // (kanode_create switches it on where the table is admissible)
    int fused_step = 1, fused_solve = 1, fused_solve_cap = 0;
    int grid_rhs = 0, grid_vjp = 0, grid_vstep = 0, vstep_rows = 1;
    int pair_vjp = 1, pair_fuse = 1, pair_persist = 1, pair_persist_s = 0;
    int adj_fused_finish = 0;
    int pair_persist_max_wg = 0, pair_persist_abort = 0;
    int last_adjoint = KANODE_ADJ_NONE;
    int chain_wide = 1, record_adj_steps = 0, fk_loop = 1, fsens_wide = 0, train_any_chain = 0;
    int last_eval = KANODE_EVAL_NONE;
};

enum OptionKind {
    OPT_FLAG,       // 0 or 1
    OPT_COUNT,      // 0..hi
    OPT_ONE_OF,     // PAIR_PERSIST_S: the kernel is instantiated for 4, 8 and 16 points per workgroup (0: its default)
    OPT_READ_ONLY   // set by the library (kanode_internal_set_last_adjoint, served)
};
struct OptionRow {
    int32_t id;
    const char* name;   // as the messages print it
    OptionKind kind;
    int64_t hi;         // OPT_COUNT's upper bound
    int HandleOptions::*field;
};
// one row per kanode_option, in the enum's order
inline constexpr OptionRow kOptionTable[] = {
    // the one special row: 1 needs the table constants (options_set's table_available)
    {KANODE_OPT_POINTWISE_TABLE, "POINTWISE_TABLE", OPT_FLAG, 1, &HandleOptions::pp_on},
    {KANODE_OPT_FUSED_STEP, "FUSED_STEP", OPT_FLAG, 1, &HandleOptions::fused_step},
    {KANODE_OPT_FUSED_SOLVE, "FUSED_SOLVE", OPT_FLAG, 1, &HandleOptions::fused_solve},
    {KANODE_OPT_FUSED_SOLVE_CAP, "FUSED_SOLVE_CAP", OPT_COUNT, 1 << 20, &HandleOptions::fused_solve_cap},   // 0 = the kernel's block
    // persistent-grid overrides of the table kernels (0 = the occupancy-derived default)
    {KANODE_OPT_GRID_RHS, "GRID_RHS", OPT_COUNT, 1 << 24, &HandleOptions::grid_rhs},
    {KANODE_OPT_GRID_VJP, "GRID_VJP", OPT_COUNT, kSlabBlocks / 2, &HandleOptions::grid_vjp},
    {KANODE_OPT_GRID_ADJ_STEP, "GRID_ADJ_STEP", OPT_COUNT, kSlabBlocks / 2, &HandleOptions::grid_vstep},
    {KANODE_OPT_ADJ_STEP_ROWS, "ADJ_STEP_ROWS", OPT_FLAG, 1, &HandleOptions::vstep_rows},
    {KANODE_OPT_PAIR_VJP, "PAIR_VJP", OPT_FLAG, 1, &HandleOptions::pair_vjp},
    {KANODE_OPT_PAIR_FUSE, "PAIR_FUSE", OPT_FLAG, 1, &HandleOptions::pair_fuse},
    {KANODE_OPT_PAIR_PERSIST, "PAIR_PERSIST", OPT_FLAG, 1, &HandleOptions::pair_persist},
    {KANODE_OPT_PAIR_PERSIST_S, "PAIR_PERSIST_S", OPT_ONE_OF, 16, &HandleOptions::pair_persist_s},   // 0: the kernel's default
    {KANODE_OPT_ADJ_FUSED_FINISH, "ADJ_FUSED_FINISH", OPT_FLAG, 1, &HandleOptions::adj_fused_finish},   // measured even with the finish launch
    {KANODE_OPT_PAIR_PERSIST_MAX_WG, "PAIR_PERSIST_MAX_WG", OPT_COUNT, 1 << 20, &HandleOptions::pair_persist_max_wg},   // 0: the device's co-resident capacity
    {KANODE_OPT_PAIR_PERSIST_ABORT, "PAIR_PERSIST_ABORT", OPT_FLAG, 1, &HandleOptions::pair_persist_abort},   // tests: raise the abort word at launch
    {KANODE_OPT_LAST_ADJOINT, "LAST_ADJOINT", OPT_READ_ONLY, 0, &HandleOptions::last_adjoint},
    {KANODE_OPT_CHAIN_WIDE, "CHAIN_WIDE", OPT_FLAG, 1, &HandleOptions::chain_wide},
    {KANODE_OPT_RECORD_ADJOINT_STEPS, "RECORD_ADJOINT_STEPS", OPT_FLAG, 1, &HandleOptions::record_adj_steps},
    {KANODE_OPT_FK_DEVICE_LOOP, "FK_DEVICE_LOOP", OPT_FLAG, 1, &HandleOptions::fk_loop},
    {KANODE_OPT_FSENS_WIDE, "FSENS_WIDE", OPT_COUNT, 2, &HandleOptions::fsens_wide},
    {KANODE_OPT_TRAIN_ANY_CHAIN, "TRAIN_ANY_CHAIN", OPT_FLAG, 1, &HandleOptions::train_any_chain},
    {KANODE_OPT_LAST_EVAL, "LAST_EVAL", OPT_READ_ONLY, 0, &HandleOptions::last_eval},
};

inline const OptionRow* option_row(int32_t id) {
    for (const OptionRow& r : kOptionTable)
        if (r.id == id) return &r;
    return nullptr;
}

// A refused set leaves the old value in place and fills msg; msg is untouched on success.
inline kanode_status options_set(HandleOptions& o, int32_t id, int64_t value, bool table_available, std::string& msg) {
    const OptionRow* r = option_row(id);
    if (!r) {
        msg = "unknown option " + std::to_string(id);
        return KANODE_ERR_INVALID_ARG;
    }
    const char* takes = nullptr;   // what a refusal says after the name
    switch (r->kind) {
    case OPT_FLAG: takes = value == 0 || value == 1 ? nullptr : " takes 0 or 1"; break;
    case OPT_COUNT: takes = value >= 0 && value <= r->hi ? nullptr : " takes 0.."; break;
    case OPT_ONE_OF: takes = value == 0 || value == 4 || value == 8 || value == 16 ? nullptr : " takes 0 (default), 4, 8 or 16"; break;
    case OPT_READ_ONLY: takes = " is read-only"; break;
    }
    if (takes) {
        msg = std::string(r->name) + takes + (r->kind == OPT_COUNT ? std::to_string(r->hi) : "");
        return KANODE_ERR_INVALID_ARG;
    }
    if (id == KANODE_OPT_POINTWISE_TABLE && value == 1 && !table_available) {
        msg = "POINTWISE_TABLE needs a pointwise f64 RHS with rbf/rswaf basis and even nx";
        return KANODE_ERR_UNSUPPORTED;
    }
    o.*(r->field) = (int)value;
    return KANODE_OK;
}

// the current value, or -1 for an unknown option
inline int64_t options_get(const HandleOptions& o, int32_t id) {
    const OptionRow* r = option_row(id);
    return r ? o.*(r->field) : -1;
}

// The largest n in [0, hi] with fits(n), for a monotone fits (true up to some n, false above); 0 when nothing fits
// (fits(0) is never asked).  The training loops' "largest capacity that still fits in LDS" searches.
template <class Pred>
inline int64_t largest_fitting(int64_t hi, Pred&& fits) {
    int64_t lo = 0;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) / 2;
        if (fits(mid)) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

#pragma GCC visibility pop
