// ensemble_args_test.cpp — the host code that lays out an ensemble launch's buffer and forms the per-replica
// argument structs (csrc/kan_ensemble.hpp).  A stand-alone host program: built with -fsanitize=address,undefined
// by tests/test_host_ensemble.py.  The "device" buffer is a host allocation of exactly ensemble_bytes(), and every
// block a replica is given is written end to end, so an offset past the buffer or two blocks that overlap fail
// the run.
#include "kan_ensemble.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {

// the fields of kan::ChainTrainArgs that ensemble_fill_args sets, and two it must copy from the shared struct
struct Args {
    double tf;
    int64_t n_save;
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

void test_layout() {
    // one replica, no private block: out | args | meta, each at a multiple of 64
    kan::EnsembleLayout L = kan::ensemble_layout(1, 0, 200);
    CHECK(L.off_rec == 64 && L.rec_stride == 0 && L.off_args == 64 && L.off_meta == 320);
    CHECK(kan::ensemble_bytes(L, 100) == 320 + 100 + 64);
    // five replicas: 80 bytes of status words round to 128; a 100-byte block takes a 128-byte stride
    L = kan::ensemble_layout(5, 100, 200);
    CHECK(L.off_rec == 128 && L.rec_stride == 128 && L.off_args == 128 + 5 * 128 && L.off_meta == 1792);
    // the largest ensemble with the largest dense-output block: no overflow, blocks in order
    const size_t rec = sizeof(double) * (1024 * 14 + 2);
    L = kan::ensemble_layout(4096, rec, 416);
    CHECK(L.off_rec == 4096 * 16 && L.rec_stride >= rec && L.rec_stride % 64 == 0);
    CHECK(L.off_args == L.off_rec + 4096 * L.rec_stride && L.off_meta >= L.off_args + 4096 * 416 && L.off_meta % 64 == 0);
}

// fills the structs of R replicas over real arrays and writes every block each replica was given
void run_fill(int64_t R, int64_t P, int64_t K, size_t rec_bytes, bool with_test, bool records, bool with_l1) {
    const kan::EnsembleLayout L = kan::ensemble_layout(R, rec_bytes, sizeof(Args));
    const size_t meta_bytes = 24;
    std::vector<char> buf(kan::ensemble_bytes(L, meta_bytes), 0);
    const size_t n = (size_t)(R * P), nk = (size_t)(R * K);
    std::vector<double> p(n), m(n), v(n), loss(nk), loss_test(nk), grad(nk * P), pb(nk * P), eta(R), l1(R), bt(2 * R);
    std::vector<int64_t> counts(nk * 4);
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
    e.l1 = with_l1 ? l1.data() : nullptr;
    e.beta_t = bt.data();
    e.loss = loss.data();
    e.loss_test = with_test ? loss_test.data() : nullptr;
    e.grad = records ? grad.data() : nullptr;
    e.p_before = records ? pb.data() : nullptr;
    e.counts = records ? counts.data() : nullptr;
    Args shared{};
    shared.tf = 3.5;
    shared.n_save = 35;
    shared.saveat = reinterpret_cast<const double*>(buf.data() + L.off_meta);
    shared.loss_test = with_test ? loss_test.data() : nullptr;
    shared.eta = -1.0;       // (per-replica fields of the shared struct are not what a replica gets)
    shared.act_reg = -1.0;
    std::vector<Args> args((size_t)R);
    kan::ensemble_fill_args(shared, e, L, buf.data(), args.data());
    // the structs themselves fit between the private blocks and the meta
    CHECK(L.off_args + (size_t)R * sizeof(Args) <= L.off_meta);
    std::memcpy(buf.data() + L.off_args, args.data(), (size_t)R * sizeof(Args));
    for (int64_t r = 0; r < R; ++r) {
        const Args& a = args[(size_t)r];
        CHECK(a.tf == 3.5 && a.n_save == 35 && a.saveat == shared.saveat);
        CHECK(a.eta == eta[r] && a.bp1 == bt[2 * r] && a.bp2 == bt[2 * r + 1] && a.act_reg == (with_l1 ? l1[r] : 0.0));
        CHECK(a.p == p.data() + r * P && a.m == m.data() + r * P && a.v == v.data() + r * P);
        CHECK(a.loss == loss.data() + r * K);
        CHECK(with_test ? a.loss_test == loss_test.data() + r * K : a.loss_test == nullptr);
        CHECK(records ? a.grad == grad.data() + r * K * P && a.p_before == pb.data() + r * K * P &&
                            a.counts == counts.data() + r * K * 4
                      : !a.grad && !a.p_before && !a.counts);
        CHECK((char*)a.out == buf.data() + 16 * r);
        // every block, written end to end with the replica's number + 1: in bounds (ASan) and, below, disjoint
        const double tag = (double)(r + 1);
        for (int64_t q = 0; q < P; ++q) a.p[q] = a.m[q] = a.v[q] = tag;
        for (int64_t k = 0; k < K; ++k) a.loss[k] = tag;
        if (a.loss_test)
            for (int64_t k = 0; k < K; ++k) a.loss_test[k] = tag;
        if (records)
            for (int64_t k = 0; k < K * P; ++k) a.grad[k] = a.p_before[k] = tag;
        if (records)
            for (int64_t k = 0; k < K * 4; ++k) a.counts[k] = r + 1;
        a.out[0] = a.out[1] = r + 1;
        if (rec_bytes) {
            CHECK((char*)a.rec == buf.data() + L.off_rec + (size_t)r * L.rec_stride);
            for (size_t k = 0; k < rec_bytes / sizeof(double); ++k) a.rec[k] = tag;
        } else {
            CHECK(a.rec == nullptr);
        }
    }
    // nobody's block was overwritten by a later replica, and the meta and the structs are as they were
    for (int64_t r = 0; r < R; ++r) {
        const Args& a = args[(size_t)r];
        const double tag = (double)(r + 1);
        CHECK(a.p[0] == tag && a.p[P - 1] == tag && a.v[P - 1] == tag && a.loss[0] == tag && a.loss[K - 1] == tag);
        CHECK(a.out[0] == r + 1 && a.out[1] == r + 1);
        if (rec_bytes) CHECK(a.rec[0] == tag && a.rec[rec_bytes / sizeof(double) - 1] == tag);
        if (records) CHECK(a.grad[0] == tag && a.grad[K * P - 1] == tag && a.counts[K * 4 - 1] == r + 1);
    }
    CHECK(std::memcmp(buf.data() + L.off_args, args.data(), (size_t)R * sizeof(Args)) == 0);
    for (size_t k = 0; k < meta_bytes + 64; ++k) CHECK(buf[L.off_meta + k] == 0);
}

}  // namespace

int main() {
    test_layout();
    run_fill(1, 240, 3, 0, false, false, false);
    run_fill(3, 240, 3, sizeof(double) * (7 * 2 * 40 + 2), true, true, true);   // (a 40-step dense-output block)
    run_fill(7, 11, 2, sizeof(double) * 16 * 128, false, true, false);          // (the Fisher-KPP accumulators)
    run_fill(259, 5, 1, 8, true, false, true);
    std::puts("ensemble_args_test ok");
    return 0;
}
