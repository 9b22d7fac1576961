// traj_grad_args_test.cpp — the host code that lays out a trajectory-ensemble gradient call (csrc/kan_ensemble.hpp:
// traj_grad_layout, the private blocks, the rows, the status words, the group size and the summation order of the
// reduction).  A stand-alone host program: built with -fsanitize=address,undefined by tests/test_host_traj_grad.py.
// Every buffer is a host allocation of exactly the size the layout asks for and every entry a trajectory is given is
// written, so an offset past a buffer or two trajectories that share an entry fail the run.
//
// With arguments `chunks R` it prints the reduction's chunk bounds for R trajectories, one "begin end" line per chunk
// (tests/test_traj_grad_cpu.py compares them with its numpy restatement of the order).
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

void test_constants() {
    CHECK(kan::traj_grad_row_elems(96) == 97 && kan::traj_grad_status_word(3) == 24);
    CHECK(kan::traj_grad_u0_elem(65535, 16, 15) == (size_t)65536 * 16 - 1);
    CHECK(kan::traj_grad_save_elem(2, 4, 9, 3, 1) == (size_t)(2 * 9 + 4) * 3 + 1);
    CHECK(kan::traj_grad_save_elem(4999, 65535, 65536, 16, 15) == (size_t)5000 * 65536 * 16 - 1);   // past 2^31
    // a private block: the dense output, k1_0, u_save / dl, the gathered target rows
    CHECK(kan::traj_grad_block_usave(2, 10) == 142 && kan::traj_grad_block_target(2, 10, 35) == 212);
    CHECK(kan::traj_grad_block_elems(2, 10, 35) == 282);
    CHECK(kan::traj_grad_host_bytes(9) == 9 * 64 + 8);
}

// the summation order: chunks of 64 consecutive trajectories, the last one shorter, every trajectory in exactly one
void test_chunks() {
    const int64_t Rs[] = {1, 9, 63, 64, 65, 128, 1030, 65536};
    for (int64_t R : Rs) {
        const int64_t nc = kan::traj_grad_chunks(R);
        CHECK(nc == (R + 63) / 64);
        int64_t next = 0;
        for (int64_t c = 0; c < nc; ++c) {
            CHECK(kan::traj_grad_chunk_begin(c) == next && kan::traj_grad_chunk_begin(c) == 64 * c);
            const int64_t e = kan::traj_grad_chunk_end(c, R);
            CHECK(e > next && e - next <= kan::kTrajGradChunk && (c + 1 == nc ? e == R : e - next == 64));
            next = e;
        }
        CHECK(next == R);
    }
    CHECK(kan::traj_grad_chunks(1030) == 17 && kan::traj_grad_chunk_end(16, 1030) - kan::traj_grad_chunk_begin(16) == 6);
}

// the group size: a multiple of the chunk, within the budget for every R, and monotone in the block size
void test_group() {
    const size_t budget = kan::kEnsembleBudget;
    const int64_t P = 240;
    int64_t last = kan::kTrajGradMax + 1;
    const size_t blocks[] = {1000, 115000, 917000, 3000000};
    for (size_t bb : blocks) {
        const size_t meta = kan::traj_grad_meta_bound(35);
        const int64_t G = kan::traj_grad_group(P, bb, meta, budget);
        CHECK(G >= 0 && G <= kan::kTrajGradMax && G % kan::kTrajGradChunk == 0 && G <= last);
        last = G;
        if (G == 0) continue;
        const int64_t Rs[] = {1, G, G + 1, kan::kTrajGradMax};
        for (int64_t R : Rs) {
            const kan::TrajGradLayout L = kan::traj_grad_layout(R, R < G ? R : G, P, bb, meta);
            CHECK(L.bytes <= budget);
        }
        // one more chunk would not fit at the largest call
        if (G < kan::kTrajGradMax)
            CHECK(kan::traj_grad_layout(kan::kTrajGradMax, G + 2 * kan::kTrajGradChunk, P, bb, meta).bytes > budget);
    }
    CHECK(kan::traj_grad_group(P, 1000, 0, budget) == kan::kTrajGradMax);
    CHECK(kan::traj_grad_group(P, (size_t)8 << 20, 0, budget) == 0);   // fewer than 64 fit: not covered
    CHECK(kan::traj_grad_group(P, 1000, 0, 1000) == 0);
}

// R trajectories in groups of G over a real buffer: every trajectory writes its status words, its row and every
// double of its block; the chunk sums of every group land in the call's chunk rows
void run(int64_t R, int64_t G, int64_t P, int64_t N, int64_t cap, int64_t n_save) {
    const size_t meta_bytes = kan::traj_grad_meta_bound(n_save);
    const size_t block_bytes = sizeof(double) * kan::traj_grad_block_elems(N, cap, n_save);
    const int64_t Gn = R < G ? R : G;
    const kan::TrajGradLayout L = kan::traj_grad_layout(R, Gn, P, block_bytes, meta_bytes);
    const size_t W = kan::traj_grad_row_elems(P);
    CHECK(L.off_loss == (size_t)R * 64 && L.off_part % 64 == 0 && L.off_rows % 64 == 0 && L.off_blocks % 64 == 0);
    CHECK(L.block_stride % 64 == 0 && L.block_stride >= block_bytes && L.off_meta % 64 == 0);
    CHECK(L.off_part >= L.off_loss + 8 && L.off_rows >= L.off_part + (size_t)kan::traj_grad_chunks(R) * W * 8);
    CHECK(L.off_blocks >= L.off_rows + (size_t)Gn * W * 8 && L.off_meta + meta_bytes + 64 <= L.bytes);
    CHECK(kan::traj_grad_host_bytes(R) == L.off_loss + 8);
    std::vector<char> buf(L.bytes, 0);
    int64_t* const status = reinterpret_cast<int64_t*>(buf.data());
    double* const part = reinterpret_cast<double*>(buf.data() + L.off_part);
    double* const rows = reinterpret_cast<double*>(buf.data() + L.off_rows);
    std::memset(buf.data() + L.off_meta, 0x5a, meta_bytes);
    CHECK(G % kan::kTrajGradChunk == 0 || G >= R);
    for (int64_t g0 = 0; g0 < R; g0 += G) {
        const int64_t Rg = R - g0 < G ? R - g0 : G;
        std::memset(rows, 0, (size_t)Gn * W * 8);
        for (int64_t r = 0; r < Rg; ++r) {
            int64_t* w = status + kan::traj_grad_status_word(g0 + r);
            CHECK((char*)(w + kan::kTrajGradStatusWords) <= buf.data() + L.off_loss);
            for (int q = 0; q < kan::kTrajGradStatusWords; ++q) {
                CHECK(w[q] == 0);
                w[q] = g0 + r + 1;
            }
            double* row = rows + (size_t)r * W;
            CHECK((char*)(row + W) <= buf.data() + L.off_blocks);
            for (size_t q = 0; q < W; ++q) {
                CHECK(row[q] == 0.0);
                row[q] = (double)(g0 + r + 1);
            }
            double* blk = reinterpret_cast<double*>(buf.data() + L.off_blocks + (size_t)r * L.block_stride);
            const size_t ne = kan::traj_grad_block_elems(N, cap, n_save);
            CHECK((char*)(blk + ne) <= buf.data() + L.off_meta);
            CHECK(kan::traj_grad_block_usave(N, cap) < kan::traj_grad_block_target(N, cap, n_save));
            for (size_t q = 0; q < ne; ++q) blk[q] = (double)(g0 + r);
        }
        // the group's chunk sums: local chunk c is the call's chunk g0 / 64 + c
        double* gp = part + (size_t)(g0 / kan::kTrajGradChunk) * W;
        for (int64_t c = 0; c < kan::traj_grad_chunks(Rg); ++c) {
            CHECK((char*)(gp + (size_t)(c + 1) * W) <= buf.data() + L.off_rows);
            for (size_t q = 0; q < W; ++q) {
                double s = 0.0;
                for (int64_t r = kan::traj_grad_chunk_begin(c); r < kan::traj_grad_chunk_end(c, Rg); ++r)
                    s = s + rows[(size_t)r * W + q];
                CHECK(gp[(size_t)c * W + q] == 0.0);
                gp[(size_t)c * W + q] = s;
            }
        }
    }
    // every chunk of the call holds the sum of its own trajectories' numbers, whatever the grouping
    for (int64_t c = 0; c < kan::traj_grad_chunks(R); ++c) {
        double want = 0.0;
        for (int64_t r = kan::traj_grad_chunk_begin(c); r < kan::traj_grad_chunk_end(c, R); ++r) want += (double)(r + 1);
        for (size_t q = 0; q < W; ++q) CHECK(part[(size_t)c * W + q] == want);
    }
    for (int64_t r = 0; r < R; ++r) CHECK(status[8 * r] == r + 1 && status[8 * r + 7] == r + 1);
    for (size_t k = 0; k < meta_bytes; ++k) CHECK(buf[L.off_meta + k] == 0x5a);
    for (size_t k = L.off_loss; k < L.off_part; ++k) CHECK(buf[k] == 0);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 3 && std::strcmp(argv[1], "chunks") == 0) {
        const int64_t R = std::atoll(argv[2]);
        for (int64_t c = 0; c < kan::traj_grad_chunks(R); ++c)
            std::printf("%lld %lld\n", (long long)kan::traj_grad_chunk_begin(c), (long long)kan::traj_grad_chunk_end(c, R));
        return 0;
    }
    test_constants();
    test_chunks();
    test_group();
    run(1, 64, 96, 2, 4, 35);
    run(9, 64, 96, 3, 22, 35);
    run(65, 64, 96, 2, 8, 3);        // two groups, the second of one trajectory
    run(1030, 256, 240, 2, 16, 5);   // five groups, 17 chunks
    run(1030, 65536, 48, 16, 2, 2);  // one group
    std::puts("traj_grad_args_test ok");
    return 0;
}
