// fit_ensemble_groups_test.cpp — the launch groups of kanode_fit_ensemble_tsit5 (csrc/kan_ensemble.hpp):
// ensemble_group, the largest replica count whose buffer stays within a budget, ensemble_slice, a group's part of
// the caller's dense arrays, and ensemble_fill_args with the one-workgroup training kernel's private-block size over
// two groups.  A stand-alone host program: built with -fsanitize=address,undefined by
// tests/test_host_fit_ensemble.py.  Each group's "device" buffer is a host allocation of exactly ensemble_bytes(),
// and every block a replica is given is written end to end, so an offset past an array or two blocks that overlap
// fail the run.
#include "kan_ensemble.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {

struct Args {
    double tf;
    const double* saveat;
    double eta, bp1, bp2, act_reg;
    double *p, *m, *v, *rec, *loss, *loss_test, *grad, *p_before;
    int64_t *counts, *out;
};

#define CHECK(c)                                                           \
    do {                                                                   \
        if (!(c)) {                                                        \
            std::fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

// the private block of kd_chain_train_wg_kernel in bytes: [cap][7][n] | k1_0 [n] | u_save [n_save][n] | the test
// u_save [n_save_test][n], rounded to 64 as the launch rounds it
size_t wg_rec_bytes(int64_t n, int64_t cap, int64_t n_save, int64_t n_save_test) {
    return kan::ensemble_round(sizeof(double) * (size_t)((cap * 7 + 1) * n + (n_save + n_save_test) * n));
}

// the definition, replica by replica
int64_t group_by_scan(int64_t R, size_t rec, size_t arg, size_t meta, size_t budget) {
    int64_t g = 0;
    while (g < R && kan::ensemble_bytes(kan::ensemble_layout(g + 1, rec, arg), meta) <= budget) ++g;
    return g;
}

void test_group() {
    // a 100-byte block (stride 128), 200-byte structs, 100 bytes of meta.  By hand, bytes(R) = round64(round64(16 R)
    // + 128 R + 200 R) + 100 + 64:  R = 1: 64 + 128 + 200 = 392 -> 448, + 164 = 612;  R = 2: 64 + 256 + 400 = 720 ->
    // 768, + 164 = 932;  R = 3: 64 + 384 + 600 = 1048 -> 1088, 1252;  R = 4: 64 + 512 + 800 = 1376 -> 1408, 1572;
    // R = 5: 128 + 640 + 1000 = 1768 -> 1792, 1956
    const size_t at[6] = {0, 612, 932, 1252, 1572, 1956};
    for (int64_t g = 1; g <= 5; ++g) {
        CHECK(kan::ensemble_bytes(kan::ensemble_layout(g, 100, 200), 100) == at[g]);
        CHECK(kan::ensemble_group(4096, 100, 200, 100, at[g]) == g);           // exactly enough
        CHECK(kan::ensemble_group(4096, 100, 200, 100, at[g] - 1) == g - 1);   // one byte short
    }
    // a budget smaller than one replica: 0, also at R = 1
    CHECK(kan::ensemble_group(1, 100, 200, 100, 611) == 0);
    CHECK(kan::ensemble_group(4096, 100, 200, 100, 0) == 0);
    // never more than R
    CHECK(kan::ensemble_group(1, 100, 200, 100, 612) == 1 && kan::ensemble_group(1, 100, 200, 100, 1u << 30) == 1);
    CHECK(kan::ensemble_group(3, 100, 200, 100, 1u << 30) == 3 && kan::ensemble_group(3, 100, 200, 100, 1251) == 2);
    CHECK(kan::ensemble_group(4096, 100, 200, 100, 1u << 30) == 4096);
    CHECK(kan::ensemble_group(0, 100, 200, 100, 1u << 30) == 0 && kan::ensemble_group(-3, 100, 200, 100, 1u << 30) == 0);
    // 4096 replicas need round64(65536 + 4096·328) + 164 = 1409024 + 164
    CHECK(kan::ensemble_group(4096, 100, 200, 100, 1409188) == 4096);
    CHECK(kan::ensemble_group(4096, 100, 200, 100, 1409187) == 4095);
    // the real sizes: 1024 steps of 32 state entries and 35 saveat rows are (7169·32 + 35·32)·8 = 1844224 bytes a
    // replica; with 416-byte structs 145 replicas take round64(2368 + 145·1844640) + meta + 64 < 2^28 <= 146 replicas'
    const size_t rec = wg_rec_bytes(32, 1024, 35, 0), meta = kan::ensemble_meta_bound(35, 0);
    CHECK(rec == 1844224 && meta == 71 * 8 + 73 * 4);
    CHECK(kan::kEnsembleBudget == (size_t)1 << 28);
    CHECK(kan::ensemble_group(4096, rec, 416, meta, kan::kEnsembleBudget) == 145);
    CHECK(kan::ensemble_group(3, rec, 416, meta, kan::kEnsembleBudget) == 3);
    CHECK(kan::ensemble_group(1, rec, 416, meta, kan::kEnsembleBudget) == 1);
    // and against the definition, over budgets around every flip of a mid-sized case
    for (size_t budget = 0; budget < 12000; budget += 7)
        for (int64_t R : {1, 3, 9, 4096})
            CHECK(kan::ensemble_group(R, 520, 416, 77, budget) == group_by_scan(R, 520, 416, 77, budget));
}

// R replicas in groups of the size a budget allows: every group laid out and filled as the C entry does it, every
// block written end to end; then every replica's blocks still carry its own tag
void run_groups(int64_t R, int64_t P, int64_t K, size_t rec_bytes, size_t budget, int64_t want_groups) {
    const size_t meta_bytes = kan::ensemble_meta_bound(35, 0);
    const int64_t G = kan::ensemble_group(4096, rec_bytes, sizeof(Args), meta_bytes, budget);
    CHECK(G >= 1);
    const size_t n = (size_t)(R * P), nk = (size_t)(R * K);
    std::vector<double> p(n), m(n), v(n), loss(nk), loss_test(nk), grad(nk * P), pb(nk * P), eta(R), l1(R), bt(2 * R);
    std::vector<int64_t> counts(nk * 4), res(2 * R, -1);
    for (int64_t r = 0; r < R; ++r) {
        eta[r] = 1e-3 * (double)(r + 1);
        l1[r] = 1e-4 * (double)r;
        bt[2 * r] = 0.9 / (double)(r + 1);
        bt[2 * r + 1] = 0.999 / (double)(r + 1);
    }
    kan::EnsembleReplicas e{};
    e.R = R;
    e.P = P;
    e.n_iters = K;
    e.p = p.data();
    e.m = m.data();
    e.v = v.data();
    e.eta = eta.data();
    e.l1 = l1.data();
    e.beta_t = bt.data();
    e.loss = loss.data();
    e.loss_test = loss_test.data();
    e.grad = grad.data();
    e.p_before = pb.data();
    e.counts = counts.data();
    int64_t groups = 0;
    std::vector<std::vector<char>> bufs;   // (kept: the second group's buffer must not be the first one's memory)
    std::vector<std::vector<Args>> all;
    for (int64_t g0 = 0; g0 < R; g0 += G, ++groups) {
        const kan::EnsembleReplicas s = kan::ensemble_slice(e, g0, G);
        CHECK(s.R == (R - g0 < G ? R - g0 : G) && s.R >= 1 && s.P == P && s.n_iters == K);
        const kan::EnsembleLayout L = kan::ensemble_layout(s.R, rec_bytes, sizeof(Args));
        CHECK(kan::ensemble_bytes(L, meta_bytes) <= budget);
        bufs.emplace_back(kan::ensemble_bytes(L, meta_bytes), 0);
        std::vector<char>& buf = bufs.back();
        Args shared{};
        shared.tf = 3.5;
        shared.saveat = reinterpret_cast<const double*>(buf.data() + L.off_meta);
        shared.loss_test = loss_test.data();
        all.emplace_back((size_t)s.R);
        std::vector<Args>& args = all.back();
        kan::ensemble_fill_args(shared, s, L, buf.data(), args.data());
        CHECK(L.off_args + (size_t)s.R * sizeof(Args) <= L.off_meta);
        for (int64_t j = 0; j < s.R; ++j) {
            const int64_t r = g0 + j;   // the replica's number in the caller's arrays
            const Args& a = args[(size_t)j];
            const double tag = (double)(r + 1);
            CHECK(a.tf == 3.5 && a.saveat == shared.saveat);
            CHECK(a.eta == eta[r] && a.bp1 == bt[2 * r] && a.bp2 == bt[2 * r + 1] && a.act_reg == l1[r]);
            CHECK(a.p == p.data() + r * P && a.m == m.data() + r * P && a.v == v.data() + r * P);
            CHECK(a.loss == loss.data() + r * K && a.loss_test == loss_test.data() + r * K);
            CHECK(a.grad == grad.data() + r * K * P && a.p_before == pb.data() + r * K * P);
            CHECK(a.counts == counts.data() + r * K * 4);
            // inside the group's buffer, and ahead of the next replica's block (or of the structs)
            CHECK((char*)a.out == buf.data() + 16 * j && (char*)(a.out + 2) <= buf.data() + L.off_rec);
            CHECK((char*)a.rec == buf.data() + L.off_rec + (size_t)j * L.rec_stride);
            CHECK((char*)a.rec + rec_bytes <= (j + 1 < s.R ? (char*)args[(size_t)j + 1].rec : buf.data() + L.off_args));
            for (int64_t q = 0; q < P; ++q) a.p[q] = a.m[q] = a.v[q] = tag;
            for (int64_t k = 0; k < K; ++k) a.loss[k] = a.loss_test[k] = tag;
            for (int64_t k = 0; k < K * P; ++k) a.grad[k] = a.p_before[k] = tag;
            for (int64_t k = 0; k < K * 4; ++k) a.counts[k] = r + 1;
            for (size_t k = 0; k < rec_bytes / sizeof(double); ++k) a.rec[k] = tag;
            a.out[0] = a.out[1] = r + 1;
        }
        // the status words of the group go to the caller's dense [R][2] at the group's offset
        std::memcpy(res.data() + 2 * g0, buf.data(), (size_t)s.R * 2 * sizeof(int64_t));
        for (size_t k = 0; k < meta_bytes + 64; ++k) CHECK(buf[L.off_meta + k] == 0);
    }
    CHECK(groups == want_groups);
    int64_t r = 0;
    for (size_t g = 0; g < all.size(); ++g)
        for (size_t j = 0; j < all[g].size(); ++j, ++r) {
            const Args& a = all[g][j];
            const double tag = (double)(r + 1);
            CHECK(a.p[0] == tag && a.p[P - 1] == tag && a.m[0] == tag && a.v[P - 1] == tag);
            CHECK(a.loss[0] == tag && a.loss[K - 1] == tag && a.loss_test[K - 1] == tag);
            CHECK(a.grad[0] == tag && a.grad[K * P - 1] == tag && a.p_before[0] == tag && a.counts[K * 4 - 1] == r + 1);
            CHECK(a.rec[0] == tag && a.rec[rec_bytes / sizeof(double) - 1] == tag);
            CHECK(res[2 * r] == r + 1 && res[2 * r + 1] == r + 1);
        }
    CHECK(r == R);
    // the caller's arrays are covered densely: no entry was left out
    for (size_t k = 0; k < n; ++k) CHECK(p[k] != 0.0 && m[k] != 0.0 && v[k] != 0.0);
    for (size_t k = 0; k < nk; ++k) CHECK(loss[k] != 0.0 && loss_test[k] != 0.0);
}

}  // namespace

int main() {
    test_group();
    // 70 steps of 32 state entries, 35 saveat rows: (491·32 + 35·32)·8 = 134656 bytes a replica; a budget of three
    // replicas and a bit: five replicas run as 3 + 2
    const size_t rec = wg_rec_bytes(32, 70, 35, 0);
    CHECK(rec == 134656);
    run_groups(5, 161, 2, rec, 3 * (rec + sizeof(Args)) + 4096, 2);
    run_groups(3, 161, 2, rec, 3 * (rec + sizeof(Args)) + 4096, 1);    // exactly one group
    run_groups(7, 96, 1, wg_rec_bytes(2, 350, 35, 71), 1 << 20, 1);   // (a pruned net with a test problem)
    run_groups(4, 96, 1, wg_rec_bytes(2, 350, 35, 71), 2 * wg_rec_bytes(2, 350, 35, 71) + 4096, 2);
    std::puts("fit_ensemble_groups_test ok");
    return 0;
}
