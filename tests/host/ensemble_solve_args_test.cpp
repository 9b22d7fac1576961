// ensemble_solve_args_test.cpp — the host code that lays out an ensemble solve (csrc/kan_ensemble.hpp:
// ens_solve_layout, the per-replica table stride and the offsets into the caller's dense arrays).  A stand-alone host
// program: built with -fsanitize=address,undefined by tests/test_host_ensemble_solve.py.  Every buffer is a host
// allocation of exactly the size the layout asks for, and every block a replica is given is written end to end, so
// an offset past a buffer or two blocks that overlap fail the run.
#include "kan_ensemble.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {

#define CHECK(c)                                                           \
    do {                                                                   \
        if (!(c)) {                                                        \
            std::fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

void test_layout() {
    // one replica: 32 bytes of status words round to 64, five saveat values to 64, then the spare 64
    kan::EnsSolveLayout L = kan::ens_solve_layout(1, 5);
    CHECK(L.off_saveat == 64 && L.bytes == 64 + 64 + 64);
    L = kan::ens_solve_layout(3, 35);
    CHECK(L.off_saveat == 128 && L.bytes == 128 + 320 + 64);
    L = kan::ens_solve_layout(4096, 141);
    CHECK(L.off_saveat == 4096 * 32 && L.bytes >= L.off_saveat + 141 * 8 + 64 && L.bytes % 64 == 0);
    // ten coefficients of ni intervals: 80·ni bytes, a multiple of 64 only where ni is a multiple of 4
    CHECK(kan::ens_table_stride(10, 64) == 640 && kan::ens_table_stride(10, 4) == 40);
    CHECK(kan::ens_table_stride(10, 6) == 64 && kan::ens_table_stride(10, 1) == 16);
    CHECK(kan::ens_table_bytes(4096, 10, 256) == (size_t)4096 * 2560 * 8);
    CHECK(kan::ens_solve_status_word(0) == 0 && kan::ens_solve_status_word(4095) == 4 * 4095);
    CHECK(kan::ens_solve_p_elem(4095, 240) == (size_t)4095 * 240);
    // past 2^31 elements: no 32-bit product anywhere
    CHECK(kan::ens_solve_save_elem(4095, 1000, 1024) == (size_t)4095 * 1000 * 1024);
}

// R replicas over real arrays: every replica writes its status words, its table and its rows of u_save
void run(int64_t R, int64_t P, int64_t n_save, int64_t n, int ni) {
    const kan::EnsSolveLayout L = kan::ens_solve_layout(R, n_save);
    std::vector<char> buf(L.bytes, 0);
    const size_t stride = kan::ens_table_stride(10, ni);
    CHECK(stride >= (size_t)10 * ni && (stride * sizeof(double)) % 64 == 0 && stride % 2 == 0);
    CHECK(L.off_saveat % 64 == 0 && L.off_saveat >= (size_t)R * 32);
    CHECK(L.off_saveat + (size_t)n_save * sizeof(double) + 64 <= L.bytes);
    std::vector<double> tables(kan::ens_table_bytes(R, 10, ni) / sizeof(double), 0.0);
    std::vector<double> p((size_t)(R * P), 0.0), u_save((size_t)(R * n_save * n), 0.0);
    int64_t* const out = reinterpret_cast<int64_t*>(buf.data());
    double* const sv = reinterpret_cast<double*>(buf.data() + L.off_saveat);
    for (int64_t j = 0; j < n_save; ++j) sv[j] = -1.0;
    for (int64_t r = 0; r < R; ++r) {
        const double tag = (double)(r + 1);
        int64_t* w = out + kan::ens_solve_status_word(r);
        CHECK((char*)(w + kan::kEnsSolveStatusWords) <= buf.data() + L.off_saveat);
        for (int q = 0; q < kan::kEnsSolveStatusWords; ++q) w[q] = r + 1;
        double* t = tables.data() + (size_t)r * stride;
        CHECK(((size_t)r * stride * sizeof(double)) % 64 == 0);
        for (int q = 0; q < 10 * ni; ++q) t[q] = tag;
        double* pr = p.data() + kan::ens_solve_p_elem(r, P);
        for (int64_t q = 0; q < P; ++q) pr[q] = tag;
        double* us = u_save.data() + kan::ens_solve_save_elem(r, n_save, n);
        for (int64_t q = 0; q < n_save * n; ++q) us[q] = tag;
    }
    // nobody's block was overwritten by a later replica; the shared saveat list and the spare bytes are untouched
    for (int64_t r = 0; r < R; ++r) {
        const double tag = (double)(r + 1);
        const int64_t* w = out + kan::ens_solve_status_word(r);
        CHECK(w[0] == r + 1 && w[3] == r + 1);
        const double* t = tables.data() + (size_t)r * stride;
        CHECK(t[0] == tag && t[10 * ni - 1] == tag);
        for (size_t q = (size_t)10 * ni; q < stride; ++q) CHECK(t[q] == 0.0);
        const double* pr = p.data() + kan::ens_solve_p_elem(r, P);
        CHECK(pr[0] == tag && pr[P - 1] == tag);
        const double* us = u_save.data() + kan::ens_solve_save_elem(r, n_save, n);
        CHECK(us[0] == tag && us[n_save * n - 1] == tag);
    }
    for (int64_t j = 0; j < n_save; ++j) CHECK(sv[j] == -1.0);
    for (size_t k = L.off_saveat + (size_t)n_save * sizeof(double); k < L.bytes; ++k) CHECK(buf[k] == 0);
    for (size_t k = (size_t)R * 32; k < L.off_saveat; ++k) CHECK(buf[k] == 0);
}

}  // namespace

int main() {
    test_layout();
    run(1, 240, 35, 2, 64);
    run(3, 56, 71, 6, 6);       // (a table whose bytes are no multiple of 64: the stride pads it)
    run(4096, 11, 11, 26, 64);
    std::puts("ensemble_solve_args_test ok");
    return 0;
}
