// kan_ensemble.hpp — the host side of an ensemble launch of the device-resident training loops (host only, no
// HIP; the constexpr index functions of the trajectory gradient are also what its kernel calls): where each
// replica's blocks lie in the handle's training buffer, and the per-replica argument structs.
//
// The buffer of a launch of R replicas:
//     out [R][2] int64 | rec [R][rec_stride bytes] | args [R] | meta | 64 spare bytes
// every block at a multiple of 64 bytes.  out[r] are replica r's status words (iterations done, stop reason), rec
// its private block (the LV loop's global dense output, the Fisher-KPP loop's accumulators; rec_bytes = 0 where the
// kernel keeps them in LDS; the general small-chain loop's dense output and cotangent rows, always there), args the structs the workgroups read, meta the ONE copy of what all replicas share
// (saveat lists, jump groups).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace kan {

struct EnsembleLayout {
    size_t off_rec, rec_stride, off_args, off_meta;
};
inline size_t ensemble_round(size_t bytes) { return (bytes + 63) & ~(size_t)63; }
inline EnsembleLayout ensemble_layout(int64_t R, size_t rec_bytes, size_t arg_bytes) {
    EnsembleLayout L;
    L.off_rec = ensemble_round((size_t)R * 2 * sizeof(int64_t));
    L.rec_stride = ensemble_round(rec_bytes);
    L.off_args = L.off_rec + (size_t)R * L.rec_stride;
    L.off_meta = ensemble_round(L.off_args + (size_t)R * arg_bytes);
    return L;
}
// the bytes the buffer needs for this layout and a meta block of meta_bytes
inline size_t ensemble_bytes(const EnsembleLayout& L, size_t meta_bytes) { return L.off_meta + meta_bytes + 64; }

// The replicas of one launch where the private blocks are large (kanode_fit_ensemble_tsit5: a dense-output block of
// up to ~1.8 MB per replica): the largest G <= R whose buffer, laid out as above, stays within `budget` bytes; 0
// when not even one replica does.  The C entry runs R replicas in consecutive groups of G (the last one smaller),
// one launch each.  A cap on the memory a handle holds, not a tuning knob: a group that fits is never split.
constexpr size_t kEnsembleBudget = (size_t)256 << 20;
inline int64_t ensemble_group(int64_t R, size_t rec_bytes, size_t arg_bytes, size_t meta_bytes, size_t budget) {
    int64_t lo = 0, hi = R < 0 ? 0 : R;   // (the buffer's size grows with the replica count)
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo + 1) / 2;
        if (ensemble_bytes(ensemble_layout(mid, rec_bytes, arg_bytes), meta_bytes) <= budget) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}
// an upper bound of the chain loops' meta block (kanode_train.cpp: saveat, saveat_test, at most n_save + 1 stops as
// doubles; at most n_save + 3 offsets and n_save rows as int32), so that the group size depends on the list
// lengths alone
inline size_t ensemble_meta_bound(int64_t n_save, int64_t n_save_test) {
    return (size_t)(2 * n_save + n_save_test + 1) * sizeof(double) + (size_t)(2 * n_save + 3) * sizeof(int32_t);
}

// What differs between the replicas, as the C entry points receive it: p, m, v [R][P] and the outputs with their
// leading replica dimension are device arrays (the record pointers nullable), eta [R], l1 [R] (nullable: all zero)
// and beta_t [R][2] host arrays.
struct EnsembleReplicas {
    int64_t R, P, n_iters;
    double *p, *m, *v;
    const double *eta, *l1, *beta_t;
    double *loss, *loss_test, *grad, *p_before;
    int64_t* counts;
};

// replicas g0 .. g0 + G - 1 (cut at e.R) of e as an ensemble of their own: one launch group of a call
inline EnsembleReplicas ensemble_slice(const EnsembleReplicas& e, int64_t g0, int64_t G) {
    const size_t q = (size_t)g0, P = (size_t)e.P, K = (size_t)e.n_iters;
    EnsembleReplicas s = e;
    s.R = e.R - g0 < G ? e.R - g0 : G;
    s.p += q * P;
    s.m += q * P;
    s.v += q * P;
    s.eta += q;
    if (s.l1) s.l1 += q;
    s.beta_t += 2 * q;
    s.loss += q * K;
    if (s.loss_test) s.loss_test += q * K;
    if (s.grad) s.grad += q * K * P;
    if (s.p_before) s.p_before += q * K * P;
    if (s.counts) s.counts += q * K * 4;
    return s;
}

// args[r] = shared with replica r's own fields set; base is the DEVICE address of the buffer laid out by L
// (only offsets are formed from it, nothing is read through it).  Args: kan::ChainTrainArgs.
template <class Args>
void ensemble_fill_args(const Args& shared, const EnsembleReplicas& e, const EnsembleLayout& L, char* base,
                        Args* args) {
    const size_t P = (size_t)e.P, K = (size_t)e.n_iters;
    for (int64_t r = 0; r < e.R; ++r) {
        Args& a = args[r];
        const size_t q = (size_t)r;
        a = shared;
        a.p = e.p + q * P;
        a.m = e.m + q * P;
        a.v = e.v + q * P;
        a.eta = e.eta[r];
        a.act_reg = e.l1 ? e.l1[r] : 0.0;
        a.bp1 = e.beta_t[2 * r];
        a.bp2 = e.beta_t[2 * r + 1];
        a.loss = e.loss + q * K;
        a.loss_test = shared.loss_test ? e.loss_test + q * K : nullptr;
        a.grad = e.grad ? e.grad + q * K * P : nullptr;
        a.p_before = e.p_before ? e.p_before + q * K * P : nullptr;
        a.counts = e.counts ? e.counts + q * K * 4 : nullptr;
        a.rec = L.rec_stride ? reinterpret_cast<double*>(base + L.off_rec + q * L.rec_stride) : nullptr;
        a.out = reinterpret_cast<int64_t*>(base) + 2 * q;
    }
}

// ---- the ensemble solve (kanode_solve_ensemble_tsit5, kan_ens_solve.hip) ----------------------------------------
// R forward solves of one problem, workgroup r at p + r·P.  The handle's buffer of a call:
//     status [R][4] int64 (naccept, nreject, nf, stop) | saveat [n_save] doubles | 64 spare bytes
// both blocks at a multiple of 64 bytes; the Fisher-KPP field has besides one PP_PHI table per replica in a buffer
// of its own, [R][table stride] doubles, every table at a multiple of 64 bytes.  The caller's arrays are dense:
// p [R][P], u_save [R][n_save][n].
constexpr int kEnsSolveStatusWords = 4;
struct EnsSolveLayout {
    size_t off_saveat, bytes;
};
inline EnsSolveLayout ens_solve_layout(int64_t R, int64_t n_save) {
    EnsSolveLayout L;
    L.off_saveat = ensemble_round((size_t)R * kEnsSolveStatusWords * sizeof(int64_t));
    L.bytes = ensemble_round(L.off_saveat + (size_t)n_save * sizeof(double)) + 64;
    return L;
}
// replica r's status words, in int64 words from the buffer's start
inline size_t ens_solve_status_word(int64_t r) { return (size_t)r * kEnsSolveStatusWords; }
// doubles between the tables of two replicas (coef coefficients of ni intervals each), and the whole buffer's bytes
inline size_t ens_table_stride(int coef, int ni) {
    return ensemble_round((size_t)coef * (size_t)ni * sizeof(double)) / sizeof(double);
}
inline size_t ens_table_bytes(int64_t R, int coef, int ni) { return (size_t)R * ens_table_stride(coef, ni) * sizeof(double); }
// replica r's parameters and saveat rows, in elements from the start of p / u_save
inline size_t ens_solve_p_elem(int64_t r, int64_t P) { return (size_t)r * (size_t)P; }
inline size_t ens_solve_save_elem(int64_t r, int64_t n_save, int64_t n) {
    return (size_t)r * (size_t)n_save * (size_t)n;
}

// ---- the trajectory solve (kanode_solve_trajectories_tsit5, kan_traj_solve.hip) ----------------------------------
// R forward solves of one problem at one p from R initial conditions, each with its own step control, a 16-lane row
// per trajectory.  The handle's buffer of a call (its own, laid out as the ensemble solve's):
//     status [R][4] int64 (naccept, nreject, nf, stop) | saveat [n_save] doubles | 64 spare bytes
// The caller's arrays are dense and trajectory-minor, the layout a batched solve of R trajectories has: u0 [R][N],
// u_save [n_save][R][N].
constexpr int kTrajSolveStatusWords = 4;
constexpr int kTrajPerWave = 4;   // 16-lane rows of a 64-lane wave
struct TrajSolveLayout {
    size_t off_saveat, bytes;
};
inline TrajSolveLayout traj_solve_layout(int64_t R, int64_t n_save) {
    TrajSolveLayout L;
    L.off_saveat = ensemble_round((size_t)R * kTrajSolveStatusWords * sizeof(int64_t));
    L.bytes = ensemble_round(L.off_saveat + (size_t)n_save * sizeof(double)) + 64;
    return L;
}
// the host copy of the status words
inline size_t traj_solve_status_bytes(int64_t R) { return (size_t)R * kTrajSolveStatusWords * sizeof(int64_t); }
// trajectory r's status words, in int64 words from the buffer's start
inline size_t traj_solve_status_word(int64_t r) { return (size_t)r * kTrajSolveStatusWords; }
// entry j of trajectory r in u0, and in row si of u_save, in elements from the array's start
inline size_t traj_solve_u0_elem(int64_t r, int64_t N, int64_t j) { return (size_t)r * (size_t)N + (size_t)j; }
inline size_t traj_solve_save_elem(int64_t si, int64_t r, int64_t R, int64_t N, int64_t j) {
    return ((size_t)si * (size_t)R + (size_t)r) * (size_t)N + (size_t)j;
}
// one-wave workgroups of a launch of R trajectories
inline int64_t traj_solve_waves(int64_t R) { return (R + kTrajPerWave - 1) / kTrajPerWave; }

// ---- the trajectory gradient (kanode_trajectories_gradient_tsit5, kan_traj_grad.hip) -----------------------------
// R solves, losses and adjoints of one problem at one p from R initial conditions, one workgroup per trajectory, then
// the mean of the R rows in a fixed order.  The caller's arrays are the trajectory solve's: u0 [R][N], target and
// u_save [n_save][R][N].  (constexpr: the kernel states its indices with the same functions.)
//
// A call runs its R trajectories as consecutive launch groups of at most G.  The handle's buffer of a call:
//     status [R][8] int64 | loss, 1 double | part [chunks(R)][P + 1] | rows [G][P + 1] | blocks [G][block stride] | meta
// every block at a multiple of 64 bytes; status and loss are adjacent, so one copy brings both to the host.
// status[r]: the forward's naccept, nreject, nf, status, then the adjoint's four (all zero where it did not run;
// its status word is kTrajGradAdjointSkipped where the loss was not finite).  rows[r - g0] of a group: the gradient
// row, the trajectory's MSE in column P.  blocks[r - g0]: the trajectory's private block,
//     dense output [cap][7][N] | k1_0 [N] | u_save / dl [n_save][N] | target[:, r, :] gathered [n_save][N]
// meta: saveat [n_save] | stops [nstops] (doubles), joff [nstops + 2] | jrows (int32): one copy for all.
constexpr int kTrajGradStatusWords = 8;
constexpr int64_t kTrajGradAdjointSkipped = 2;
constexpr int64_t kTrajGradMax = 65536;   // trajectories of one call (kTrajMaxTrajectories)
constexpr size_t traj_grad_row_elems(int64_t P) { return (size_t)P + 1; }
constexpr size_t traj_grad_status_word(int64_t r) { return (size_t)r * kTrajGradStatusWords; }
constexpr size_t traj_grad_u0_elem(int64_t r, int64_t N, int64_t j) { return (size_t)r * (size_t)N + (size_t)j; }
constexpr size_t traj_grad_save_elem(int64_t si, int64_t r, int64_t R, int64_t N, int64_t j) {
    return ((size_t)si * (size_t)R + (size_t)r) * (size_t)N + (size_t)j;
}
// a private block, in doubles from its start
constexpr size_t traj_grad_block_usave(int64_t N, int64_t cap) { return (size_t)(cap * 7 + 1) * (size_t)N; }
constexpr size_t traj_grad_block_target(int64_t N, int64_t cap, int64_t n_save) {
    return traj_grad_block_usave(N, cap) + (size_t)n_save * (size_t)N;
}
constexpr size_t traj_grad_block_elems(int64_t N, int64_t cap, int64_t n_save) {
    return traj_grad_block_target(N, cap, n_save) + (size_t)n_save * (size_t)N;
}
// The summation order of the reduction, a function of R alone: chunk c holds the trajectories
// [chunk_begin(c), chunk_end(c, R)), kTrajGradChunk consecutive ones (the last chunk fewer).  A chunk is summed from
// 0.0 in ascending r, the chunk sums from 0.0 in ascending c, then one division by R.
constexpr int kTrajGradChunk = 64;
constexpr int64_t traj_grad_chunks(int64_t R) { return (R + kTrajGradChunk - 1) / kTrajGradChunk; }
constexpr int64_t traj_grad_chunk_begin(int64_t c) { return c * kTrajGradChunk; }
constexpr int64_t traj_grad_chunk_end(int64_t c, int64_t R) {
    return (c + 1) * kTrajGradChunk < R ? (c + 1) * kTrajGradChunk : R;
}
struct TrajGradLayout {
    size_t off_loss, off_part, off_rows, off_blocks, block_stride, off_meta, bytes;
};
// R trajectories in the call, at most G in a launch group
inline TrajGradLayout traj_grad_layout(int64_t R, int64_t G, int64_t P, size_t block_bytes, size_t meta_bytes) {
    TrajGradLayout L;
    const size_t row = traj_grad_row_elems(P) * sizeof(double);
    L.off_loss = (size_t)R * kTrajGradStatusWords * sizeof(int64_t);
    L.off_part = ensemble_round(L.off_loss + sizeof(double));
    L.off_rows = ensemble_round(L.off_part + (size_t)traj_grad_chunks(R) * row);
    L.off_blocks = ensemble_round(L.off_rows + (size_t)G * row);
    L.block_stride = ensemble_round(block_bytes);
    L.off_meta = L.off_blocks + (size_t)G * L.block_stride;
    L.bytes = ensemble_round(L.off_meta + meta_bytes) + 64;
    return L;
}
// the host copy of a call: the status words and the loss
inline size_t traj_grad_host_bytes(int64_t R) {
    return (size_t)R * kTrajGradStatusWords * sizeof(int64_t) + sizeof(double);
}
// what one more trajectory of a launch group adds to the buffer
inline size_t traj_grad_bytes_per_traj(int64_t P, size_t block_bytes) {
    return ensemble_round(block_bytes) + traj_grad_row_elems(P) * sizeof(double);
}
// The trajectories of one launch group: the most whose buffer stays within `budget` whatever R the call has (the
// status words and chunk sums are counted at kTrajGradMax), at most kTrajGradMax.  A multiple of kTrajGradChunk, so a
// chunk never straddles two groups and the chunk sums of a group can be formed right after its launch; 0 where not
// even one chunk fits.
inline int64_t traj_grad_group(int64_t P, size_t block_bytes, size_t meta_bytes, size_t budget) {
    const size_t fixed = traj_grad_layout(kTrajGradMax, 0, P, 0, meta_bytes).bytes + 128;
    if (budget <= fixed) return 0;
    int64_t G = (int64_t)((budget - fixed) / traj_grad_bytes_per_traj(P, block_bytes));
    if (G > kTrajGradMax) G = kTrajGradMax;
    return G - G % kTrajGradChunk;
}
// the chain adjoint's meta block for this saveat list, as an upper bound (ensemble_meta_bound without a test problem)
inline size_t traj_grad_meta_bound(int64_t n_save) { return ensemble_meta_bound(n_save, 0); }

// ---- the trajectory gradient in fp32 (kanode_trajectories_gradient_f32_tsit5, kan_traj_grad_f32.hip) --------------
// The same call with float arrays: the status words, the chunk order, the index functions of u0 / target / u_save and
// the meta block are the ones above; what is counted in elements of `esize` bytes is stated here with that size as an
// argument (esize = sizeof(double) gives the fp64 entry's numbers).  The handle's buffer of a call:
//     status [R][8] int64 | loss, one 8-byte slot (the float total in its first four bytes) | part [chunks(R)][P + 1]
//     | rows [G][P + 1] | blocks [G][block stride] | meta
// with part, rows and the blocks in `esize` elements.  A private block of the fp32 kernel holds no gathered target
// (the kernel reads target[:, r, :] by index):
//     dense output [cap][7][N] | k1_0 [N] | u_save / dl [n_save][N]
constexpr size_t traj_grad_f32_block_usave(int64_t N, int64_t cap) { return traj_grad_block_usave(N, cap); }
constexpr size_t traj_grad_f32_block_elems(int64_t N, int64_t cap, int64_t n_save) {
    return traj_grad_block_target(N, cap, n_save);
}
inline TrajGradLayout traj_grad_layout_es(int64_t R, int64_t G, int64_t P, size_t block_bytes, size_t meta_bytes,
                                          size_t esize) {
    TrajGradLayout L;
    const size_t row = traj_grad_row_elems(P) * esize;
    L.off_loss = (size_t)R * kTrajGradStatusWords * sizeof(int64_t);
    L.off_part = ensemble_round(L.off_loss + sizeof(double));
    L.off_rows = ensemble_round(L.off_part + (size_t)traj_grad_chunks(R) * row);
    L.off_blocks = ensemble_round(L.off_rows + (size_t)G * row);
    L.block_stride = ensemble_round(block_bytes);
    L.off_meta = L.off_blocks + (size_t)G * L.block_stride;
    L.bytes = ensemble_round(L.off_meta + meta_bytes) + 64;
    return L;
}
inline size_t traj_grad_bytes_per_traj_es(int64_t P, size_t block_bytes, size_t esize) {
    return ensemble_round(block_bytes) + traj_grad_row_elems(P) * esize;
}
// traj_grad_group's rule at this element size: a multiple of kTrajGradChunk, at most kTrajGradMax, 0 where no chunk fits
inline int64_t traj_grad_group_es(int64_t P, size_t block_bytes, size_t meta_bytes, size_t budget, size_t esize) {
    const size_t fixed = traj_grad_layout_es(kTrajGradMax, 0, P, 0, meta_bytes, esize).bytes + 128;
    if (budget <= fixed) return 0;
    int64_t G = (int64_t)((budget - fixed) / traj_grad_bytes_per_traj_es(P, block_bytes, esize));
    if (G > kTrajGradMax) G = kTrajGradMax;
    return G - G % kTrajGradChunk;
}

}  // namespace kan
