// traj_solve_args_test.cpp — the host code that lays out a trajectory solve (csrc/kan_ensemble.hpp: traj_solve_layout,
// the status words and the offsets into the caller's dense, trajectory-minor arrays).  A stand-alone host program:
// built with -fsanitize=address,undefined by tests/test_host_trajectories.py.  Every buffer is a host allocation of
// exactly the size the layout asks for, and every entry a trajectory is given is written, so an offset past a buffer
// or two trajectories that share an entry fail the run.
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
    // one trajectory: 32 bytes of status words round to 64, five saveat values to 64, then the spare 64
    kan::TrajSolveLayout L = kan::traj_solve_layout(1, 5);
    CHECK(L.off_saveat == 64 && L.bytes == 64 + 64 + 64);
    L = kan::traj_solve_layout(9, 35);
    CHECK(L.off_saveat == 320 && L.bytes == 320 + 320 + 64);
    L = kan::traj_solve_layout(65536, 141);
    CHECK(L.off_saveat == (size_t)65536 * 32 && L.bytes >= L.off_saveat + 141 * 8 + 64 && L.bytes % 64 == 0);
    CHECK(kan::traj_solve_status_bytes(65536) == (size_t)65536 * 32 && kan::traj_solve_status_bytes(1) == 32);
    CHECK(kan::traj_solve_status_word(0) == 0 && kan::traj_solve_status_word(65535) == 4 * 65535);
    CHECK(kan::traj_solve_u0_elem(0, 2, 1) == 1 && kan::traj_solve_u0_elem(65535, 16, 15) == (size_t)65536 * 16 - 1);
    // u_save is [n_save][R][N]: row si of a batched solve of R trajectories, trajectory r's N entries inside it
    CHECK(kan::traj_solve_save_elem(0, 0, 9, 2, 0) == 0 && kan::traj_solve_save_elem(1, 0, 9, 2, 0) == 18);
    CHECK(kan::traj_solve_save_elem(2, 4, 9, 3, 1) == (size_t)(2 * 9 + 4) * 3 + 1);
    // past 2^31 elements: no 32-bit product anywhere
    CHECK(kan::traj_solve_save_elem(4999, 65535, 65536, 16, 15) == (size_t)5000 * 65536 * 16 - 1);
    // four rows to a wave, the last wave partly filled
    CHECK(kan::traj_solve_waves(1) == 1 && kan::traj_solve_waves(4) == 1 && kan::traj_solve_waves(5) == 2);
    CHECK(kan::traj_solve_waves(9) == 3 && kan::traj_solve_waves(1030) == 258 && kan::traj_solve_waves(65536) == 16384);
}

// R trajectories over real arrays: every trajectory writes its status words, reads its entries of u0 and writes its
// entries of every saveat row
void run(int64_t R, int64_t N, int64_t n_save) {
    const kan::TrajSolveLayout L = kan::traj_solve_layout(R, n_save);
    std::vector<char> buf(L.bytes, 0);
    CHECK(L.off_saveat % 64 == 0 && L.off_saveat >= kan::traj_solve_status_bytes(R));
    CHECK(L.off_saveat + (size_t)n_save * sizeof(double) + 64 <= L.bytes);
    std::vector<char> host(kan::traj_solve_status_bytes(R), 0);
    std::vector<double> u0((size_t)(R * N), 0.0), u_save((size_t)(n_save * R * N), 0.0);
    int64_t* const out = reinterpret_cast<int64_t*>(buf.data());
    double* const sv = reinterpret_cast<double*>(buf.data() + L.off_saveat);
    for (int64_t j = 0; j < n_save; ++j) sv[j] = -1.0;
    for (int64_t r = 0; r < R; ++r)
        for (int64_t j = 0; j < N; ++j) {
            double& x = u0[kan::traj_solve_u0_elem(r, N, j)];
            CHECK(x == 0.0);   // (nobody else's entry)
            x = (double)(r * N + j + 1);
        }
    for (int64_t r = 0; r < R; ++r) {
        int64_t* w = out + kan::traj_solve_status_word(r);
        CHECK((char*)(w + kan::kTrajSolveStatusWords) <= buf.data() + L.off_saveat);
        for (int q = 0; q < kan::kTrajSolveStatusWords; ++q) w[q] = r + 1;
        for (int64_t si = 0; si < n_save; ++si)
            for (int64_t j = 0; j < N; ++j) {
                double& x = u_save[kan::traj_solve_save_elem(si, r, R, N, j)];
                CHECK(x == 0.0);
                x = u0[kan::traj_solve_u0_elem(r, N, j)] + (double)si;
            }
    }
    std::memcpy(host.data(), buf.data(), host.size());
    // every entry written once, in the batched solve's order; the shared saveat list and the spare bytes untouched
    for (int64_t si = 0; si < n_save; ++si)
        for (int64_t q = 0; q < R * N; ++q) CHECK(u_save[(size_t)(si * R * N + q)] == (double)(q + 1 + si));
    const int64_t* hw = reinterpret_cast<const int64_t*>(host.data());
    for (int64_t r = 0; r < R; ++r) CHECK(hw[4 * r] == r + 1 && hw[4 * r + 3] == r + 1);
    for (int64_t j = 0; j < n_save; ++j) CHECK(sv[j] == -1.0);
    for (size_t k = L.off_saveat + (size_t)n_save * sizeof(double); k < L.bytes; ++k) CHECK(buf[k] == 0);
    for (size_t k = kan::traj_solve_status_bytes(R); k < L.off_saveat; ++k) CHECK(buf[k] == 0);
}

}  // namespace

int main() {
    test_layout();
    run(1, 2, 35);
    run(9, 3, 35);        // (two full waves and one with a single live row)
    run(1030, 2, 3);
    run(65536, 16, 2);
    std::puts("traj_solve_args_test ok");
    return 0;
}
