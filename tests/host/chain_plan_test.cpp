// chain_plan_test.cpp — the launch decisions of the small-chain kernels (csrc/kan_chain_plan.hpp: the small-chain
// shape, the specialisation rung, the model / block / dynamic LDS / staging of the one-workgroup adjoint).  A
// stand-alone host program: built with -fsanitize=address,undefined by tests/test_host_chain_plan.py.
//
// Every expected value below is a literal worked out by hand from the launchers' formulas (the arithmetic is in the
// comment next to it), at the smallest case on either side of each decision.  Sizes: sizeof(LayerConst) = 1248,
// WideModel::kEnd = 672 elements, kLvP = 240, the static Jacobian stage of the stage-parallel adjoint
// jst = 8·8·2·(240 + 2) = 30,976 B; budgets 48 KB = 49,152 B, 60 KB = 61,440 B, 140 KB = 143,360 B.
#include "kan_chain_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {

#define CHECK(c)                                                           \
    do {                                                                   \
        if (!(c)) {                                                        \
            std::fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

struct LC {
    int32_t I, O, G, norm, basis, use_base, path;
};
enum { TANH_FAST = 0, TANH = 1, SOFTSIGN = 2, RBF = 0, RSWAF = 1, DIRECT = 0, REC = 1, REC_CORR = 2 };

const kan::ChainLimits K{16, 256, 64, 8, 4, 16, 1024, 16, 64, 672, 2, 10, 2, 5, 240, 1, 6, 1248,
                         TANH_FAST, SOFTSIGN, REC, REC_CORR, RBF};

// a chain of the given widths, every layer G knots, rbf, base activation on
std::vector<LC> chain(std::vector<int> dims, int G, int norm, int path) {
    std::vector<LC> v;
    for (size_t l = 0; l + 1 < dims.size(); ++l) v.push_back(LC{dims[l], dims[l + 1], G, norm, RBF, 1, path});
    return v;
}
int64_t plen(const std::vector<LC>& v) {
    int64_t P = 0;
    for (const LC& h : v) P += (int64_t)h.O * h.G * h.I + (h.use_base ? h.O * h.I : 0);
    return P;
}
kan::ChainAdjPlan plan(const std::vector<LC>& v, int64_t P, int64_t B, bool wide, int64_t steps, size_t esize,
                       bool lv_models = true) {
    return kan::chain_adjoint_plan(K, v.data(), (int)v.size(), P, B, wide, steps, esize, lv_models);
}
bool is(const kan::ChainAdjPlan& p, int model, int threads, size_t lds, int stage_rec) {
    if (p.model == model && p.threads == threads && p.lds == lds && p.stage_rec == stage_rec) return true;
    std::fprintf(stderr, "plan: model %d threads %d lds %zu stage_rec %d\n", p.model, p.threads, p.lds, p.stage_rec);
    return false;
}
bool none(const kan::ChainAdjPlan& p) { return is(p, kan::kAdjNone, 0, 0, 0); }
bool fwd_ok(const std::vector<LC>& v) { return kan::chain_small_layers(K, v.data(), (int)v.size(), K.fwd_layers); }
bool vjp_ok(const std::vector<LC>& v) { return kan::chain_small_layers(K, v.data(), (int)v.size(), K.vjp_layers); }
bool solve_ok(const std::vector<LC>& v, int64_t B, size_t esize) {
    return kan::chain_tsit5_shape(K, v.data(), (int)v.size(), plen(v), B, esize);
}
kan::ChainRung rung(const std::vector<LC>& v) { return kan::chain_rung(K, v.data(), (int)v.size()); }

void test_lotka_volterra() {
    const std::vector<LC> lv = chain({2, 10, 2}, 5, TANH_FAST, REC);
    CHECK(plen(lv) == 240 && kan::chain_is_lv(lv.data(), 2) && kan::chain_is_lv_wave(K, lv.data(), 2, 1, true));
    CHECK(fwd_ok(lv) && vjp_ok(lv) && solve_ok(lv, 1, 8) && solve_ok(lv, 16, 4));
    CHECK(kan::chain_param_lds(K, 2, 240, 8) == 4416);   // 2·1248 + 240·8
    // one trajectory, wide, fp64, P = 240: the stage-parallel model on 6 + 1 waves.
    // lsp = 2·1248 + 8·(240 + 2·45) = 5136, rec = 8·(7·45 + 1)·2 = 5056, + jst = 41,168 <= 143,360: staged
    CHECK(is(plan(lv, 240, 1, true, 45, 8), kan::kAdjLvSp, 448, 10192, 1));
    // staged while 4416 + 16 s + 112 s + 16 + 30,976 <= 143,360, i.e. s <= 843
    CHECK(is(plan(lv, 240, 1, true, 843, 8), kan::kAdjLvSp, 448, 112336, 1));   // 4416 + 13,488 + 94,416 + 16
    CHECK(is(plan(lv, 240, 1, true, 844, 8), kan::kAdjLvSp, 448, 17920, 0));    // 4416 + 13,504
    CHECK(is(plan(lv, 240, 1, true, 1024, 8), kan::kAdjLvSp, 448, 20800, 0));
    // wide off, or two trajectories: a column group each (one wave, four groups), the LV-shape rung.
    // 2·1248 + 240·8·(1 + 4 + 9) + 16 + 16·45 = 2496 + 26,880 + 16 + 720
    CHECK(is(plan(lv, 240, 1, false, 45, 8), kan::kAdjChain, 64, 30112, 0));
    CHECK(is(plan(lv, 240, 2, true, 45, 8), kan::kAdjChain, 64, 30112, 0));
    CHECK(rung(lv) == kan::kRungLV);
    // softsign: the same models, the forward on the runtime-normalizer REC rung
    const std::vector<LC> ss = chain({2, 10, 2}, 5, SOFTSIGN, REC);
    CHECK(rung(ss) == kan::kRungRec);
    CHECK(is(plan(ss, 240, 1, true, 45, 8), kan::kAdjLvSp, 448, 10192, 1));
    CHECK(is(plan(ss, 240, 2, true, 45, 8), kan::kAdjChain, 64, 30112, 0));
    // fp32: the LV wave model.  pre = 2·1248 + 4·240·10 = 12,096; staged while 12,096 + 16 s + 4·(7 s + 1)·2 <= 61,440,
    // i.e. 72 s <= 49,336, s <= 685
    CHECK(is(plan(lv, 240, 1, true, 45, 4), kan::kAdjLvWave, 64, 15344, 1));    // 12,096 + 720 + 2528
    CHECK(is(plan(lv, 240, 1, true, 685, 4), kan::kAdjLvWave, 64, 61424, 1));   // 12,096 + 10,960 + 38,368
    CHECK(is(plan(lv, 240, 1, true, 686, 4), kan::kAdjLvWave, 64, 23072, 0));   // 12,096 + 10,976
    // another normalizer, another basis: not the wave models'
    std::vector<LC> th = chain({2, 10, 2}, 5, TANH, REC);
    CHECK(!kan::chain_is_lv_wave(K, th.data(), 2, 1, true) && plan(th, 240, 1, true, 45, 8).model == kan::kAdjChain);
    std::vector<LC> rs = lv;
    rs[1].basis = RSWAF;
    CHECK(!kan::chain_is_lv_wave(K, rs.data(), 2, 1, true) && plan(rs, 240, 1, true, 45, 8).model == kan::kAdjWide);
    // a training loop without the wave models (lv_models off) gets WideModel for this shape:
    // pre = 2496 + 8·(2400 + 672) = 27,072, + 720 + rec 5056
    CHECK(is(plan(lv, 240, 1, true, 45, 8, false), kan::kAdjWide, 256, 32848, 1));
    // the stage-parallel LDS with a training loop's saveat rows beside it (extra doubles):
    // 2496 + 8·(240 + 128 + 318) = 7984, rec = 8·449·2 = 7184
    int sr = -1;
    CHECK(kan::lvsp_lds(K, 64, 318, &sr) == 15168 && sr == 1);
    // at one step: fits while 2496 + 8·(242 + e) + 30,976 <= 143,360, e <= 13,494; staged (rec 128) while e <= 13,478
    CHECK(kan::lvsp_lds(K, 1, 13478, &sr) == 112384 &&   // 2496 + 109,760 + 128
          sr == 1);
    CHECK(kan::lvsp_lds(K, 1, 13479, &sr) == 112264 && sr == 0);
    CHECK(kan::lvsp_lds(K, 1, 13494, &sr) == 112384 && sr == 0);
    CHECK(kan::lvsp_lds(K, 1, 13495, &sr) == 0 && sr == 0);
}

void test_wide_and_chain() {
    // a pruned [2,3,2]: P = 2·(3·5·2 + 6) = 72.  One trajectory, wide: the whole workgroup on it.
    // pre = 2496 + 8·(720 + 672) = 13,632; staged while 13,632 + 16 s + 112 s + 16 <= 61,440, s <= 373
    const std::vector<LC> pr = chain({2, 3, 2}, 5, TANH_FAST, REC);
    CHECK(plen(pr) == 72 && kan::chain_is_wide(K, pr.data(), 2, 1, true) && !kan::chain_is_lv(pr.data(), 2));
    CHECK(is(plan(pr, 72, 1, true, 373, 8), kan::kAdjWide, 256, 61392, 1));   // 13,632 + 5968 + 41,792
    CHECK(is(plan(pr, 72, 1, true, 374, 8), kan::kAdjWide, 256, 19616, 0));   // 13,632 + 5984
    // two trajectories: column groups.  2496 + 72·8·14 + 16 + 720
    CHECK(is(plan(pr, 72, 2, true, 45, 8), kan::kAdjChain, 64, 11296, 0));
    CHECK(is(plan(pr, 72, 1, false, 45, 8), kan::kAdjChain, 64, 11296, 0));
    CHECK(rung(pr) == kan::kRungTanhRec);
    // three layers [2,4,4,2]: P = 48 + 96 + 48; 3·1248 + 192·8·14 + 16 + 720
    const std::vector<LC> l3 = chain({2, 4, 4, 2}, 5, TANH_FAST, REC);
    CHECK(plen(l3) == 192 && is(plan(l3, 192, 1, true, 45, 8), kan::kAdjChain, 64, 25984, 0));
    // wide_fits by one: [1,2,1] with 15 knots in layer 1 has 1·16 features per hidden unit (a DPP row), with 16 it
    // has 17.  G1 = 15: P = 32 + 12, pre = 2496 + 8·(440 + 672) = 11,392, + 720 + rec 8·316 = 2528
    std::vector<LC> w = chain({1, 2, 1}, 5, SOFTSIGN, REC_CORR);
    w[0].G = 15;
    CHECK(plen(w) == 44 && is(plan(w, 44, 1, true, 45, 8), kan::kAdjWide, 256, 14640, 1));
    w[0].G = 16;   // P = 34 + 12; 2496 + 46·8·14 + 16 + 720
    CHECK(plen(w) == 46 && !kan::chain_is_wide(K, w.data(), 2, 1, true));
    CHECK(is(plan(w, 46, 1, true, 45, 8), kan::kAdjChain, 64, 8384, 0));
    CHECK(kan::wide_fits(K, 2, 16, 2, 5, 3) && !kan::wide_fits(K, 2, 16, 2, 5, 4));   // 16·4 = 64, 16·5 = 80
    CHECK(kan::wide_fits(K, 4, 4, 4, 3, 5) && !kan::wide_fits(K, 5, 4, 5, 2, 5));     // at most four outputs (waves)
    CHECK(!kan::wide_fits(K, 2, 3, 1, 5, 5));                                          // I == O
    // the 60 KB limit of the column-group model: one layer [8 -> 8], P = 8·5·8 + 64 = 384, five trajectories on two
    // waves (eight groups): 1248 + 384·8·(1 + 8 + 9) + 16 + 16 s = 56,560 + 16 s <= 61,440 while s <= 305
    const std::vector<LC> sq = chain({8, 8}, 5, TANH_FAST, REC);
    CHECK(plen(sq) == 384 && is(plan(sq, 384, 5, true, 305, 8), kan::kAdjChain, 128, 61440, 0));
    CHECK(none(plan(sq, 384, 5, true, 306, 8)));
    // fp32 on the column-group model wants the parameter rows 8-byte aligned: [3 -> 3] without the base activation has
    // P = 45, with it 54 (1248 + 54·4·14 + 16 + 160)
    std::vector<LC> odd = chain({3, 3}, 5, TANH_FAST, REC);
    CHECK(is(plan(odd, 54, 1, true, 10, 4), kan::kAdjChain, 64, 4448, 0));
    odd[0].use_base = 0;
    CHECK(plen(odd) == 45 && none(plan(odd, 45, 1, true, 10, 4)));
    CHECK(plan(odd, 45, 1, true, 10, 8).model == kan::kAdjChain);
}

void test_unsupported() {
    // five layers: the forward kernels take eight, the pullback kernels four
    const std::vector<LC> l5 = chain({2, 2, 2, 2, 2, 2}, 5, TANH_FAST, REC);
    CHECK(fwd_ok(l5) && !vjp_ok(l5) && solve_ok(l5, 1, 8) && none(plan(l5, plen(l5), 1, true, 45, 8)));
    const std::vector<LC> l4 = chain({2, 2, 2, 2, 2}, 5, TANH_FAST, REC);
    CHECK(vjp_ok(l4) && plan(l4, plen(l4), 1, true, 45, 8).model == kan::kAdjChain);
    const std::vector<LC> l9 = chain({2, 2, 2, 2, 2, 2, 2, 2, 2, 2}, 5, TANH_FAST, REC);
    CHECK(fwd_ok(chain({2, 2, 2, 2, 2, 2, 2, 2, 2}, 5, TANH_FAST, REC)) && !fwd_ok(l9));
    CHECK(!kan::chain_small_layers(K, l4.data(), 0, K.fwd_layers));
    // a layer 17 wide
    const std::vector<LC> w17 = chain({2, 17, 2}, 2, TANH_FAST, REC);
    CHECK(!fwd_ok(w17) && !vjp_ok(w17) && !solve_ok(w17, 1, 8) && none(plan(w17, plen(w17), 2, true, 45, 8)));
    CHECK(fwd_ok(chain({2, 16, 2}, 2, TANH_FAST, REC)));
    // mixed paths, mixed normalizers, layers that do not fit each other
    std::vector<LC> mp = chain({2, 10, 2}, 5, TANH_FAST, REC);
    mp[1].path = DIRECT;
    CHECK(!fwd_ok(mp) && !solve_ok(mp, 1, 8) && none(plan(mp, 240, 2, true, 45, 8)));
    std::vector<LC> mn = chain({2, 10, 2}, 5, TANH_FAST, REC);
    mn[1].norm = SOFTSIGN;
    CHECK(!fwd_ok(mn) && !solve_ok(mn, 1, 8) && none(plan(mn, 240, 1, true, 45, 8)));
    std::vector<LC> gap = chain({2, 10, 2}, 5, TANH_FAST, REC);
    gap[1].I = 9;
    CHECK(!fwd_ok(gap) && none(plan(gap, 240, 1, true, 45, 8)));
    // I != O: a layer chain, but no ODE right-hand side
    const std::vector<LC> io = chain({2, 10, 3}, 5, TANH_FAST, REC);
    CHECK(fwd_ok(io) && kan::I_ne_O(io.data(), 2) && !solve_ok(io, 1, 8) && none(plan(io, plen(io), 1, true, 45, 8)));
    // batch and step count
    const std::vector<LC> lv = chain({2, 10, 2}, 5, TANH_FAST, REC);
    CHECK(solve_ok(lv, 16, 8) && !solve_ok(lv, 17, 8) && !solve_ok(lv, 0, 8));
    CHECK(plan(lv, 240, 16, true, 45, 8).model == kan::kAdjChain && none(plan(lv, 240, 17, true, 45, 8)));
    CHECK(plan(lv, 240, 16, true, 45, 8).threads == 256 && none(plan(lv, 240, 0, true, 45, 8)));
    CHECK(plan(lv, 240, 1, true, 1024, 8).model == kan::kAdjLvSp && none(plan(lv, 240, 1, true, 1025, 8)));
    CHECK(none(plan(lv, 240, 1, true, 0, 8)));
    // the 48 KB of constants and parameters: 1248 + 8 P <= 49,152 while P <= 5988
    CHECK(kan::chain_params_fit(K, 1, 5988, 8) && !kan::chain_params_fit(K, 1, 5989, 8));
    CHECK(kan::chain_threads(K, 1) == 64 && kan::chain_threads(K, 4) == 64 && kan::chain_threads(K, 5) == 128 &&
          kan::chain_threads(K, 16) == 256);
}

void test_rungs() {
    CHECK(rung(chain({2, 10, 2}, 5, TANH_FAST, REC)) == kan::kRungLV);
    CHECK(rung(chain({2, 10, 2}, 6, TANH_FAST, REC)) == kan::kRungTanhRec);
    CHECK(rung(chain({2, 10, 2}, 5, TANH_FAST, REC_CORR)) == kan::kRungRecCorr);
    CHECK(rung(chain({2, 10, 2}, 5, SOFTSIGN, REC_CORR)) == kan::kRungRecCorr);
    CHECK(rung(chain({2, 10, 2}, 5, SOFTSIGN, REC)) == kan::kRungRec);
    CHECK(rung(chain({2, 10, 2}, 5, TANH, REC)) == kan::kRungRec);
    CHECK(rung(chain({2, 10, 2}, 5, TANH_FAST, DIRECT)) == kan::kRungDirect);
    CHECK(rung(chain({3, 3}, 5, SOFTSIGN, DIRECT)) == kan::kRungDirect);
}

}  // namespace

int main() {
    test_lotka_volterra();
    test_wide_and_chain();
    test_unsupported();
    test_rungs();
    std::puts("chain_plan_test ok");
    return 0;
}
