// traj_grad_f32_args_test.cpp — the host code that plans an fp32 trajectory-ensemble gradient call: the element-size
// layout, block and group functions of csrc/kan_ensemble.hpp and the LDS plan of csrc/kan_chain_plan.hpp
// (traj_grad_f32_carve, traj_grad_f32_lds).  A stand-alone host program: built with -fsanitize=address,undefined by
// tests/test_host_traj_grad_f32.py.  Every buffer is a host allocation of exactly the size the layout asks for and
// every entry a trajectory is given is written, so an offset past a buffer or two trajectories that share an entry
// fail the run.
#include "kan_chain_plan.hpp"
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

// the fields kan_chain_plan.hpp reads of a layer's constants
struct LC {
    int I, O, G, path, norm, use_base, basis;
};
// the device classes' numbers (kan_col.hip's kChainLimits), with a layer-constants size that is a multiple of 8
const kan::ChainLimits kLim{16, 256, 64, 8, 4, 16, 1024, 16, 64, 2048, 2, 10, 2, 5, 240, 1, 6, 512, 2, 1, 1, 2, 0};

int64_t params(const LC* l, int nl) {
    int64_t P = 0;
    for (int i = 0; i < nl; ++i) P += (int64_t)l[i].I * l[i].O * (l[i].G + l[i].use_base);
    return P;
}

void test_blocks_and_rows() {
    // a float block: the dense output, k1_0, u_save / dl; no gathered target
    CHECK(kan::traj_grad_f32_block_usave(2, 10) == 142 && kan::traj_grad_f32_block_elems(2, 10, 35) == 212);
    CHECK(kan::traj_grad_f32_block_elems(3, 1, 1) == 8 * 3 + 3);
    CHECK(kan::traj_grad_row_elems(240) == 241);
    // esize = 8 is the fp64 entry's layout, field by field
    const kan::TrajGradLayout a = kan::traj_grad_layout(1030, 256, 240, 917000, 700);
    const kan::TrajGradLayout b = kan::traj_grad_layout_es(1030, 256, 240, 917000, 700, sizeof(double));
    CHECK(a.off_loss == b.off_loss && a.off_part == b.off_part && a.off_rows == b.off_rows &&
          a.off_blocks == b.off_blocks && a.block_stride == b.block_stride && a.off_meta == b.off_meta &&
          a.bytes == b.bytes);
    CHECK(kan::traj_grad_group(240, 917000, 700, kan::kEnsembleBudget) ==
          kan::traj_grad_group_es(240, 917000, 700, kan::kEnsembleBudget, sizeof(double)));
}

// the group size at floats: a multiple of the chunk, within the budget for every R up to 65536, monotone in the block
void test_group() {
    const size_t budget = kan::kEnsembleBudget, es = sizeof(float);
    const int64_t P = 240;
    int64_t last = kan::kTrajGradMax + 1;
    const size_t blocks[] = {1000, 57500, 458500, 3000000};
    for (size_t bb : blocks) {
        const size_t meta = kan::traj_grad_meta_bound(35);
        const int64_t G = kan::traj_grad_group_es(P, bb, meta, budget, es);
        CHECK(G >= 0 && G <= kan::kTrajGradMax && G % kan::kTrajGradChunk == 0 && G <= last);
        last = G;
        if (G == 0) continue;
        const int64_t Rs[] = {1, G, G + 1, kan::kTrajGradMax};
        for (int64_t R : Rs) CHECK(kan::traj_grad_layout_es(R, R < G ? R : G, P, bb, meta, es).bytes <= budget);
        if (G < kan::kTrajGradMax)
            CHECK(kan::traj_grad_layout_es(kan::kTrajGradMax, G + 2 * kan::kTrajGradChunk, P, bb, meta, es).bytes >
                  budget);
        // half the bytes per element: never fewer trajectories than the double layout gives for the doubled block
        CHECK(G >= kan::traj_grad_group(P, 2 * bb, meta, budget));
    }
    CHECK(kan::traj_grad_group_es(P, 1000, 0, budget, es) == kan::kTrajGradMax);
    CHECK(kan::traj_grad_group_es(P, (size_t)8 << 20, 0, budget, es) == 0);   // fewer than 64 fit: not covered
    CHECK(kan::traj_grad_group_es(P, 1000, 0, 1000, es) == 0);
}

// R trajectories in groups of G over a real buffer: every trajectory writes its status words, its float row and every
// float of its block; the chunk sums of every group land in the call's chunk rows
void run(int64_t R, int64_t G, int64_t P, int64_t N, int64_t cap, int64_t n_save) {
    const size_t es = sizeof(float);
    const size_t meta_bytes = kan::traj_grad_meta_bound(n_save);
    const size_t ne = kan::traj_grad_f32_block_elems(N, cap, n_save);
    const size_t block_bytes = es * ne;
    const int64_t Gn = R < G ? R : G;
    const kan::TrajGradLayout L = kan::traj_grad_layout_es(R, Gn, P, block_bytes, meta_bytes, es);
    const size_t W = kan::traj_grad_row_elems(P);
    CHECK(L.off_loss == (size_t)R * 64 && L.off_part % 64 == 0 && L.off_rows % 64 == 0 && L.off_blocks % 64 == 0);
    CHECK(L.block_stride % 64 == 0 && L.block_stride >= block_bytes && L.off_meta % 64 == 0);
    CHECK(L.off_part >= L.off_loss + 8 && L.off_rows >= L.off_part + (size_t)kan::traj_grad_chunks(R) * W * es);
    CHECK(L.off_blocks >= L.off_rows + (size_t)Gn * W * es && L.off_meta + meta_bytes + 64 <= L.bytes);
    CHECK(L.off_meta == L.off_blocks + (size_t)Gn * L.block_stride);
    CHECK(kan::traj_grad_host_bytes(R) == L.off_loss + 8);
    // the block holds its parts, in order and without overlap
    CHECK(kan::traj_grad_f32_block_usave(N, cap) == (size_t)(cap * 7 + 1) * N);
    CHECK(ne == kan::traj_grad_f32_block_usave(N, cap) + (size_t)n_save * N);
    std::vector<char> buf(L.bytes, 0);
    int64_t* const status = reinterpret_cast<int64_t*>(buf.data());
    float* const part = reinterpret_cast<float*>(buf.data() + L.off_part);
    float* const rows = reinterpret_cast<float*>(buf.data() + L.off_rows);
    std::memset(buf.data() + L.off_meta, 0x5a, meta_bytes);
    CHECK(G % kan::kTrajGradChunk == 0 || G >= R);
    for (int64_t g0 = 0; g0 < R; g0 += G) {
        const int64_t Rg = R - g0 < G ? R - g0 : G;
        std::memset(rows, 0, (size_t)Gn * W * es);
        for (int64_t r = 0; r < Rg; ++r) {
            int64_t* w = status + kan::traj_grad_status_word(g0 + r);
            CHECK((char*)(w + kan::kTrajGradStatusWords) <= buf.data() + L.off_loss);
            for (int q = 0; q < kan::kTrajGradStatusWords; ++q) {
                CHECK(w[q] == 0);
                w[q] = g0 + r + 1;
            }
            float* row = rows + (size_t)r * W;
            CHECK((char*)(row + W) <= buf.data() + L.off_blocks);
            for (size_t q = 0; q < W; ++q) {
                CHECK(row[q] == 0.0f);
                row[q] = (float)((g0 + r) % 512 + 1);
            }
            float* blk = reinterpret_cast<float*>(buf.data() + L.off_blocks + (size_t)r * L.block_stride);
            CHECK((char*)(blk + ne) <= buf.data() + L.off_meta);
            for (size_t q = 0; q < ne; ++q) blk[q] = (float)(g0 + r);
        }
        float* gp = part + (size_t)(g0 / kan::kTrajGradChunk) * W;
        for (int64_t c = 0; c < kan::traj_grad_chunks(Rg); ++c) {
            CHECK((char*)(gp + (size_t)(c + 1) * W) <= buf.data() + L.off_rows);
            for (size_t q = 0; q < W; ++q) {
                float s = 0.0f;
                for (int64_t r = kan::traj_grad_chunk_begin(c); r < kan::traj_grad_chunk_end(c, Rg); ++r)
                    s = s + rows[(size_t)r * W + q];
                CHECK(gp[(size_t)c * W + q] == 0.0f);
                gp[(size_t)c * W + q] = s;
            }
        }
    }
    // every chunk of the call holds the sum of its own trajectories' numbers (small integers: exact in float)
    for (int64_t c = 0; c < kan::traj_grad_chunks(R); ++c) {
        float want = 0.0f;
        for (int64_t r = kan::traj_grad_chunk_begin(c); r < kan::traj_grad_chunk_end(c, R); ++r)
            want += (float)(r % 512 + 1);
        for (size_t q = 0; q < W; ++q) CHECK(part[(size_t)c * W + q] == want);
    }
    for (int64_t r = 0; r < R; ++r) CHECK(status[8 * r] == r + 1 && status[8 * r + 7] == r + 1);
    for (size_t k = 0; k < meta_bytes; ++k) CHECK(buf[L.off_meta + k] == 0x5a);
    for (size_t k = L.off_loss; k < L.off_part; ++k) CHECK(buf[k] == 0);
}

// the LDS carve: parts in order, the doubles at multiples of 8 bytes, every byte of a real allocation written once
void carve(int64_t P, int64_t cap, int64_t n_save, int64_t n, int dl) {
    const kan::TrajGradF32Carve c = kan::traj_grad_f32_carve(P, 4, cap, n_save, n, dl);
    CHECK(c.ps == 0 && c.work == 4 * (size_t)P && c.mu == c.work + 16 * (size_t)P && c.km == c.mu + 8 * (size_t)P);
    CHECK(c.gl == c.km + 28 * (size_t)P && c.tsl == c.gl + 4 * (size_t)P && c.dtsl == c.tsl + 8 * (size_t)cap);
    CHECK(c.sv == c.dtsl + 8 * (size_t)cap && c.dl == c.sv + 8 * (size_t)n_save);
    CHECK(c.total == c.dl + (dl ? 4 * (size_t)(n_save * n) : 0));
    if (P % 2 == 0) CHECK(c.tsl % 8 == 0 && c.dtsl % 8 == 0 && c.sv % 8 == 0 && c.dl % 4 == 0);
    std::vector<unsigned char> lds(c.total, 0);
    auto fill = [&](size_t off, size_t bytes) {
        CHECK(off + bytes <= lds.size());
        for (size_t k = 0; k < bytes; ++k) {
            CHECK(lds[off + k] == 0);
            lds[off + k] = 1;
        }
    };
    fill(c.ps, 4 * P), fill(c.work, 4 * (4 * P + 9 * P)), fill(c.gl, 4 * P);   // (rows, μ and kμ: zeroed as one run)
    fill(c.tsl, 8 * cap), fill(c.dtsl, 8 * cap), fill(c.sv, 8 * n_save);
    if (dl) fill(c.dl, 4 * n_save * n);
    for (unsigned char b : lds) CHECK(b == 1);
}

void test_lds_plan() {
    const LC lv[2] = {{2, 10, 5, 1, 2, 1, 0}, {10, 2, 5, 1, 2, 1, 0}};      // [2,10,2], P = 240
    const LC s4[2] = {{3, 6, 5, 1, 2, 1, 0}, {6, 3, 5, 1, 2, 1, 0}};        // [3,6,3], P = 216
    const LC wide[2] = {{2, 20, 5, 1, 2, 1, 0}, {20, 2, 5, 1, 2, 1, 0}};    // a layer wider than 16
    const LC odd[1] = {{1, 1, 2, 1, 2, 1, 0}};                               // KDense(1, 1, 2): P = 3
    const LC io[2] = {{2, 4, 5, 1, 2, 1, 0}, {4, 3, 5, 1, 2, 1, 0}};        // n_in != n_out
    CHECK(params(lv, 2) == 240 && params(s4, 2) == 216 && params(odd, 1) == 3);
    int dl = -1;
    // the largest capacity fits with u_save in LDS, within the budget; the plan is the column-group adjoint on a wave
    for (const LC* l : {lv, s4}) {
        const int64_t P = params(l, 2), n = l[0].I;
        for (int64_t cap : {1, 64, 350, 1024}) {
            const size_t lds = kan::traj_grad_f32_lds(kLim, l, 2, P, cap, 35, &dl);
            CHECK(lds > 0 && lds <= kan::kOneWgBudget && dl == 1);
            CHECK(lds == 2 * kLim.lc_bytes + kan::traj_grad_f32_carve(P, 4, cap, 35, n, 1).total);
            const kan::ChainAdjPlan plan = kan::chain_adjoint_plan(kLim, l, 2, P, 1, false, cap, sizeof(float), false);
            CHECK(plan.model == kan::kAdjChain && plan.threads == 64);
            // the kernel's carve holds what chain_group_adjoint_lds counts, the gradient and the saveat rows besides
            CHECK(lds + 16 >= plan.lds);
        }
        CHECK(kan::traj_grad_f32_lds(kLim, l, 2, P, 1025, 35, &dl) == 0 && dl == 0);   // more steps than the adjoint holds
        CHECK(kan::traj_grad_f32_lds(kLim, l, 2, P, 0, 35, &dl) == 0);
    }
    // a saveat list too long for u_save in LDS: u_save goes to the block; longer still: no fit
    const size_t big = kan::traj_grad_f32_lds(kLim, lv, 2, 240, 1024, 3000, &dl);
    CHECK(big > 0 && big <= kan::kOneWgBudget && dl == 0);
    CHECK(kan::traj_grad_f32_lds(kLim, lv, 2, 240, 1024, 6000, &dl) == 0 && dl == 0);
    // refusals: odd P, a wide layer, n_in != n_out
    CHECK(kan::traj_grad_f32_lds(kLim, odd, 1, 3, 64, 35, &dl) == 0 && dl == 0);
    CHECK(kan::traj_grad_f32_lds(kLim, wide, 2, params(wide, 2), 64, 35, &dl) == 0);
    CHECK(kan::traj_grad_f32_lds(kLim, io, 2, params(io, 2), 64, 35, &dl) == 0);
    carve(240, 1024, 35, 2, 1);
    carve(240, 1024, 35, 2, 0);
    carve(216, 7, 3, 3, 1);
    carve(2, 1, 1, 1, 1);
}

}  // namespace

int main() {
    test_blocks_and_rows();
    test_group();
    test_lds_plan();
    run(1, 64, 96, 2, 4, 35);
    run(9, 64, 96, 3, 22, 35);
    run(65, 64, 96, 2, 8, 3);        // two groups, the second of one trajectory
    run(1030, 256, 240, 2, 16, 5);   // five groups, 17 chunks
    run(1030, 65536, 48, 16, 2, 2);  // one group
    // the buffer at the group size for R = 65536, the LV chain at the largest capacity
    {
        const size_t bb = sizeof(float) * kan::traj_grad_f32_block_elems(2, 1024, 35), meta = kan::traj_grad_meta_bound(35);
        const int64_t G = kan::traj_grad_group_es(240, bb, meta, kan::kEnsembleBudget, sizeof(float));
        CHECK(G >= 64 && G % 64 == 0);
        CHECK(kan::traj_grad_layout_es(65536, G, 240, bb, meta, sizeof(float)).bytes <= kan::kEnsembleBudget);
        std::printf("group %lld\n", (long long)G);
    }
    std::puts("traj_grad_f32_args_test ok");
    return 0;
}
