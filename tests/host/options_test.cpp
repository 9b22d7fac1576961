// options_test.cpp — the handle's option table (csrc/kanode_options.hpp: options_set / options_get, which
// kanode_set_option / kanode_get_option call) and largest_fitting, the training loops' capacity search.  A stand-alone
// host program: built with -fsanitize=address,undefined by tests/test_host_options.py.
//
// Every expected value below is a literal from include/kanode.h's documentation of the option (its default, its
// values) and the library's stated bounds (FUSED_SOLVE_CAP and PAIR_PERSIST_MAX_WG up to 2^20 = 1,048,576, GRID_RHS up
// to 2^24 = 16,777,216, GRID_VJP and GRID_ADJ_STEP up to half the 4096 slab rows = 2048, FSENS_WIDE 0..2); nothing is
// read back from the table under test.
#include "kanode_options.hpp"

#include <cstdio>
#include <cstdlib>
#include <string>

namespace {

#define CHECK(c)                                                           \
    do {                                                                   \
        if (!(c)) {                                                        \
            std::fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

struct Case {
    int32_t id;
    int64_t dflt;
    int64_t lo, hi;           // both ends of the accepted range
    int64_t bad_lo, bad_hi;   // the first refused value on each side
    const char* msg;          // what a refusal says
};

// (POINTWISE_TABLE's default is 0 on a fresh option set: kanode_create switches it on where the table is admissible)
const Case kCases[] = {
    {1, 0, 0, 1, -1, 2, "POINTWISE_TABLE takes 0 or 1"},
    {2, 1, 0, 1, -1, 2, "FUSED_STEP takes 0 or 1"},
    {3, 1, 0, 1, -1, 2, "FUSED_SOLVE takes 0 or 1"},
    {4, 0, 0, 1048576, -1, 1048577, "FUSED_SOLVE_CAP takes 0..1048576"},
    {5, 0, 0, 16777216, -1, 16777217, "GRID_RHS takes 0..16777216"},
    {6, 0, 0, 2048, -1, 2049, "GRID_VJP takes 0..2048"},
    {7, 0, 0, 2048, -1, 2049, "GRID_ADJ_STEP takes 0..2048"},
    {8, 1, 0, 1, -1, 2, "ADJ_STEP_ROWS takes 0 or 1"},
    {9, 1, 0, 1, -1, 2, "PAIR_VJP takes 0 or 1"},
    {10, 1, 0, 1, -1, 2, "PAIR_FUSE takes 0 or 1"},
    {11, 1, 0, 1, -1, 2, "PAIR_PERSIST takes 0 or 1"},
    {12, 0, 0, 16, -1, 17, "PAIR_PERSIST_S takes 0 (default), 4, 8 or 16"},
    {13, 0, 0, 1, -1, 2, "ADJ_FUSED_FINISH takes 0 or 1"},
    {14, 0, 0, 1048576, -1, 1048577, "PAIR_PERSIST_MAX_WG takes 0..1048576"},
    {15, 0, 0, 1, -1, 2, "PAIR_PERSIST_ABORT takes 0 or 1"},
    // 16 = LAST_ADJOINT: read-only, below
    {17, 1, 0, 1, -1, 2, "CHAIN_WIDE takes 0 or 1"},
    {18, 0, 0, 1, -1, 2, "RECORD_ADJOINT_STEPS takes 0 or 1"},
    {19, 1, 0, 1, -1, 2, "FK_DEVICE_LOOP takes 0 or 1"},
    {20, 0, 0, 2, -1, 3, "FSENS_WIDE takes 0..2"},
    {21, 0, 0, 1, -1, 2, "TRAIN_ANY_CHAIN takes 0 or 1"},
    // 22 = LAST_EVAL: read-only, below
};

void refused(HandleOptions& o, int32_t id, int64_t value, kanode_status want, const char* text, int64_t kept) {
    std::string msg;
    CHECK(options_set(o, id, value, true, msg) == want);
    if (msg != text) std::fprintf(stderr, "option %d value %lld: \"%s\"\n", id, (long long)value, msg.c_str());
    CHECK(msg == text);
    CHECK(options_get(o, id) == kept);   // the old value stays
}

void accepted(HandleOptions& o, int32_t id, int64_t value) {
    std::string msg;
    CHECK(options_set(o, id, value, true, msg) == KANODE_OK);
    CHECK(msg.empty());   // no message is built on success
    CHECK(options_get(o, id) == value);
}

void test_ranges() {
    for (const Case& c : kCases) {
        HandleOptions o;
        CHECK(options_get(o, c.id) == c.dflt);
        accepted(o, c.id, c.lo);
        refused(o, c.id, c.bad_lo, KANODE_ERR_INVALID_ARG, c.msg, c.lo);
        accepted(o, c.id, c.hi);
        refused(o, c.id, c.bad_hi, KANODE_ERR_INVALID_ARG, c.msg, c.hi);
        refused(o, c.id, c.bad_lo, KANODE_ERR_INVALID_ARG, c.msg, c.hi);
        // no other option moved
        const HandleOptions fresh;
        for (const Case& d : kCases)
            if (d.id != c.id) CHECK(options_get(o, d.id) == options_get(fresh, d.id));
    }
}

void test_special_rows() {
    HandleOptions o;
    // LAST_ADJOINT: KANODE_ADJ_NONE = 0 until the library records a path; never settable
    CHECK(options_get(o, 16) == 0);
    refused(o, 16, 0, KANODE_ERR_INVALID_ARG, "LAST_ADJOINT is read-only", 0);
    refused(o, 16, 1, KANODE_ERR_INVALID_ARG, "LAST_ADJOINT is read-only", 0);
    o.last_adjoint = 3;   // (as kanode_internal_set_last_adjoint does)
    CHECK(options_get(o, 16) == 3);
    // LAST_EVAL: KANODE_EVAL_NONE = 0 until a call is served; never settable; its own field
    CHECK(options_get(o, 22) == 0);
    refused(o, 22, 0, KANODE_ERR_INVALID_ARG, "LAST_EVAL is read-only", 0);
    refused(o, 22, 4, KANODE_ERR_INVALID_ARG, "LAST_EVAL is read-only", 0);
    o.last_eval = KANODE_EVAL_FK_POINT;   // (as served() does)
    CHECK(options_get(o, 22) == 7);
    CHECK(options_get(o, 16) == 3);
    o.last_adjoint = 0;
    CHECK(options_get(o, 22) == 7);
    // the eight paths, as include/kanode.h numbers them
    CHECK(KANODE_EVAL_NONE == 0 && KANODE_EVAL_CHAIN_KERNEL == 1 && KANODE_EVAL_CHAIN_STEP == 2 &&
          KANODE_EVAL_CHAIN_ADJ_STEP == 3 && KANODE_EVAL_PER_LAYER == 4 && KANODE_EVAL_PAIR == 5 &&
          KANODE_EVAL_FK_TABLE == 6 && KANODE_EVAL_FK_POINT == 7);
    // PAIR_PERSIST_S: the instantiated workgroup sizes and 0
    const int64_t good[] = {0, 4, 8, 16}, bad[] = {1, 2, 5, 32};
    for (int64_t v : good) accepted(o, 12, v);
    for (int64_t v : bad) refused(o, 12, v, KANODE_ERR_INVALID_ARG, "PAIR_PERSIST_S takes 0 (default), 4, 8 or 16", 16);
    // POINTWISE_TABLE = 1 needs the table; 0 never does; a bad value is INVALID_ARG either way
    std::string msg;
    CHECK(options_set(o, 1, 1, false, msg) == KANODE_ERR_UNSUPPORTED);
    CHECK(msg == "POINTWISE_TABLE needs a pointwise f64 RHS with rbf/rswaf basis and even nx");
    CHECK(options_get(o, 1) == 0);
    msg.clear();
    CHECK(options_set(o, 1, 2, false, msg) == KANODE_ERR_INVALID_ARG);
    CHECK(msg == "POINTWISE_TABLE takes 0 or 1");
    msg.clear();
    CHECK(options_set(o, 1, 1, true, msg) == KANODE_OK && msg.empty());
    CHECK(options_get(o, 1) == 1);
    CHECK(options_set(o, 1, 0, false, msg) == KANODE_OK && msg.empty());
    CHECK(options_get(o, 1) == 0);
    // unknown ids on either side of the enum
    const int32_t unknown[] = {0, 23};
    const char* text[] = {"unknown option 0", "unknown option 23"};
    for (int q = 0; q < 2; ++q) {
        msg.clear();
        CHECK(options_set(o, unknown[q], 0, true, msg) == KANODE_ERR_INVALID_ARG);
        CHECK(msg == text[q]);
        CHECK(options_get(o, unknown[q]) == -1);
    }
}

// exactly one row per enum value 1..22: no gap, no duplicate, no two options sharing a field
void test_table_shape() {
    int seen[23] = {};
    int rows = 0;
    for (const OptionRow& r : kOptionTable) {
        CHECK(r.id >= 1 && r.id <= 22);
        ++seen[r.id];
        ++rows;
        for (const OptionRow& q : kOptionTable) CHECK(&q == &r || q.field != r.field);
    }
    CHECK(rows == 22);
    for (int id = 1; id <= 22; ++id) CHECK(seen[id] == 1);
}

// fits = "n <= k": the answer is min(k, hi), and 0 when nothing fits
int64_t upto(int64_t hi, int64_t k) {
    return largest_fitting(hi, [k](int64_t n) { return n <= k; });
}
void test_largest_fitting() {
    const int64_t hi = 1024;
    CHECK(largest_fitting(hi, [](int64_t) { return true; }) == 1024);
    CHECK(largest_fitting(hi, [](int64_t) { return false; }) == 0);
    CHECK(upto(hi, 0) == 0);
    CHECK(upto(hi, 1) == 1);
    CHECK(upto(hi, 1023) == 1023);
    CHECK(upto(hi, 1024) == 1024);
    CHECK(upto(hi, 5000) == 1024);
    CHECK(upto(7, 3) == 3);   // (an odd interval)
    // hi = 0: nothing to ask; hi = 1: one question
    CHECK(largest_fitting(0, [](int64_t) { return true; }) == 0);
    CHECK(largest_fitting(0, [](int64_t) { return false; }) == 0);
    CHECK(largest_fitting(1, [](int64_t) { return true; }) == 1);
    CHECK(largest_fitting(1, [](int64_t) { return false; }) == 0);
    // the predicate is never asked outside [1, hi]
    largest_fitting(hi, [hi](int64_t n) {
        CHECK(n >= 1 && n <= hi);
        return n <= 100;
    });
}

}  // namespace

int main() {
    test_ranges();
    test_special_rows();
    test_table_shape();
    test_largest_fitting();
    std::printf("options_test ok\n");
    return 0;
}
