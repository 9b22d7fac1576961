// chain_record_probe.cpp — what csrc/kan_chain_plan.hpp itself says about the records of tests/chain_cases.py.  A
// stand-alone host program, built and run by tests/test_chain_cases_cpu.py: the case table states every record's
// rung and launchers by hand, and this program is the header's side of that comparison (the Python restatement of the
// rules is a third).
//
// Reads one record per line from the file named on the command line:
//     id esize P B nl  then per layer: I O G norm path        (the enumerators of kan_device.hpp)
// and prints per record:
//     id small8 small4 fit rung vjp_lds n_ne batch_ok
// small8 / small4: chain_small_layers at the forward kernels' and the pullback kernels' layer caps; fit:
// chain_params_fit (the forward kernel's 48 KiB); rung: chain_rung; vjp_lds: launch_kd_chain_vjp_stage's LDS test,
// nl·sizeof(LayerConst) + P·esize·(1 + block / dim groups) <= 60 KiB with kChainVjpBlock = 64; n_ne: I_ne_O;
// batch_ok: B <= 32,768 (launch_kd_chain_col).  The limits are those kan_col.hip fills in (kChainLimits).
#include "kan_chain_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {

struct LC {
    int32_t I, O, G, norm, basis, use_base, path;
};

// kChainDim 16, kChainBlock 256, kWave 64, kMaxLayers 8, kChainMaxLayers 4, kChainSolveMaxBatch 16,
// kChainAdjointMaxSteps 1024, kWideF1 16, kWideF2 64, WideModel::kEnd 672, the LV shape 2 / 10 / 2 / G 5, kLvP 240,
// KAN_LV_SP 1, kLvSpWaves 6, sizeof(LayerConst) 1248, NORM_TANH_FAST 0, NORM_SOFTSIGN 2, PATH_REC 1, PATH_REC_CORR 2,
// BASIS_RBF 0
const kan::ChainLimits K{16, 256, 64, 8, 4, 16, 1024, 16, 64, 672, 2, 10, 2, 5, 240, 1, 6, 1248, 0, 2, 1, 2, 0};
constexpr int kVjpBlock = 64;        // kChainVjpBlock
constexpr long kFwdMaxBatch = 32768;

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: chain_record_probe RECORDS\n");
        return 2;
    }
    std::FILE* in = std::fopen(argv[1], "r");
    if (!in) {
        std::perror(argv[1]);
        return 2;
    }
    char id[128];
    long esize, P, B;
    int nl, n = 0;
    while (std::fscanf(in, "%127s %ld %ld %ld %d", id, &esize, &P, &B, &nl) == 5) {
        if (nl < 1 || nl > 8 || (esize != 4 && esize != 8) || P < 1 || B < 1) {
            std::fprintf(stderr, "%s: bad record\n", id);
            return 2;
        }
        std::vector<LC> v((size_t)nl);
        for (LC& h : v) {
            if (std::fscanf(in, "%d %d %d %d %d", &h.I, &h.O, &h.G, &h.norm, &h.path) != 5) {
                std::fprintf(stderr, "%s: short record\n", id);
                return 2;
            }
            h.basis = 0;
            h.use_base = 1;
        }
        const int groups = kVjpBlock / K.dim;
        const size_t vjp_lds = (size_t)nl * K.lc_bytes + (size_t)P * (size_t)esize * (size_t)(1 + groups);
        std::printf("%s %d %d %d %d %d %d %d\n", id, (int)kan::chain_small_layers(K, v.data(), nl, K.fwd_layers),
                    (int)kan::chain_small_layers(K, v.data(), nl, K.vjp_layers),
                    (int)kan::chain_params_fit(K, nl, P, (size_t)esize), (int)kan::chain_rung(K, v.data(), nl),
                    (int)(vjp_lds <= kan::kOneWgBudget), (int)kan::I_ne_O(v.data(), nl), (int)(B <= kFwdMaxBatch));
        ++n;
    }
    std::fclose(in);
    std::fprintf(stderr, "chain_record_probe: %d records\n", n);
    return n > 0 ? 0 : 2;
}
