// dojo_data_adjoint.hpp -- reverse sweep over the recorded IFT Jacobians of a rollout for the gradient of a trajectory loss w.r.t. the CONTACT DATA
// (dojo_rollout_data_adjoint_dev).  The per-step derivative is get_contact_gradients (src/gradients/contact.jl:1-55); the reference chains it forward,
// step by step, on the host (examples/system_identification/utilities.jl:42-90) -- this is the same chain, transposed, in one launch.
//
// theta = [friction_coefficient, contact_radius, contact_origin(3)] per contact, in mechanism.contacts order: nth = 5 Nc values.  It is mechanism data,
// shared by all environments of a handle (one theta per environment would put the contact table on the batch axis of the step kernel: not built).
//
// Per environment b, with g_k the cotangent of the loss w.r.t. the state after step k (tangent coordinates, as in dojo_adjoint.hpp):
//
//     lambda <- g_{H-1};  a <- 0
//     for k = H-1 .. 0:   failed step (status[k][b] != 0):  lambda <- 0                                  (by select: DZ_k, DC_k are never read)
//                         else:                             a <- a + DC_k[b]^T lambda,   lambda <- DZ_k[b]^T lambda
//                         if k > 0: lambda <- lambda + g_{k-1}
//     gtheta_env[b] <- a;   gz[b] <- lambda;   gtheta <- sum_b a_b
//
// DC is in the layout dojo_contact_gradients_dev writes: [H][B][5Nc][nx], column-major per environment like DZ, so that (DC^T lambda)[c] is the dot
// product of a contiguous column with lambda -- "a block of columns of nx rows behind DZ", which is what adjoint::Columns calls DU.  The sweep is
// therefore rollout_adjoint_kernel with DC in DU's place, on the same step loop (adjoint::sweep: the same loads, the same waits, the same summation
// order inside a column).  What differs is where a finished column goes, i.e. the `put` this kernel hands to the loop: a
// column c >= nx is ADDED to the fp64 accumulator a[c - nx] in LDS (5Nc doubles next to lambda and g).  An accumulator is written by exactly one lane
// per step and the barrier that ends a step orders the steps, so the order of the additions over k is fixed (H-1 down to 0): no atomics.  Which lane
// owns a column may differ at step 0 (gz == NULL: the columns of the step then start at nx) -- the accumulators live in LDS, not in registers, for that.
// At the end a is rounded once into gtheta_env [B][5Nc] and / or left as fp64 in a workspace [B][5Nc]; the sum over the batch is then
// data_reduce_kernel: one workgroup of 256 lanes per entry, lane t adds the environments t, t + 256, ... in ascending order and the 256 sums meet in a
// tree (adjoint::row_sum inside every DPP row, the sixteen row sums through LDS into one more row_sum): an order fixed by B alone, of depth
// ceil(log2 B) for B <= 256; rounded once.  (The shared policy's reduction, padjoint::policy_reduce_kernel, gives a lane every sixteenth environment:
// with the few entries there are here that is two workgroups walking B / 16 dependent additions.)  gtheta_env and gz do not depend on where an
// environment sits in the batch; gtheta is bit-identical from run to run.
//
// The gradient w.r.t. the controls is not an output: a third column block would be a change to adjoint::Columns / issue, and DU is a small share of the
// traffic (nx nu next to nx^2).  A caller who wants both runs dojo_rollout_adjoint_dev over the same record (dojo_rollout_data_gradients does).
#pragma once
#include <hip/hip_runtime.h>
#include "dojo_math.hpp"
#include "dojo_adjoint.hpp"

namespace dj {
namespace dadjoint {

constexpr int THREADS = adjoint::THREADS;
static_assert(adjoint::TEAMS == adjoint::ROW, "data_reduce_kernel sums the row sums of a workgroup in one DPP row");

template <class TIO> struct Args {
    const TIO* DZ;          // [H][B][nx][nx]
    const TIO* DC;          // [H][B][nth][nx] (unused when neither gtheta_env nor acc_out is wanted)
    const TIO* G;           // [H][B][nx] (cot_space 0) or [H][B][13 Nb] (cot_space 1)
    const TIO* Z;           // [H][B][13 Nb], cot_space 1 only
    const int* status;      // [H][B] or null
    TIO* gtheta_env;        // [B][nth] or null
    double* acc_out;        // [B][nth] fp64 workspace in front of the reduction over the batch, or null
    TIO* gz;                // [B][nx] or null
    int H, B, nx, nth, cot_space;
};

inline size_t lds_bytes(int nx, int nth) { return ((size_t)4 * nx + (size_t)nth) * sizeof(double); }     // lambda and g, double-buffered; the accumulators

#if defined(__HIPCC__)
template <class TIO>
__global__ void __launch_bounds__(THREADS) rollout_data_adjoint_kernel(const Args<TIO> A) {
    using namespace adjoint;
    extern __shared__ __align__(16) double lds_[];                          // lambda [2][nx] | g [2][nx] | a [nth]
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
    const int nx = A.nx, nth = (A.gtheta_env || A.acc_out) ? A.nth : 0;
    TIO* const gz = DJ_GLOBAL_PTR(TIO, A.gz);
    const Columns<TIO> C = columns<TIO>(DJ_GLOBAL_PTR(const TIO, A.DZ), DJ_GLOBAL_PTR(const TIO, A.DC), A.B, nx, A.nth, nth);
    double* const lam_ = lds_; double* const a_ = lds_ + 4 * nx;

    for (int e = tid; e < nth; e += THREADS) a_[e] = 0.0;
    for (int c = tid; c < nx; c += THREADS) lam_[c] = 0.0;
    sweep(C, cot_of<TIO>(A), DJ_GLOBAL_PTR(const int, A.status), A.H, b, lam_, lds_ + 2 * nx,
        // the columns of step k: [c0, nx) of DZ (lambda; step 0 feeds gz alone), then the nth columns of DC (the accumulators)
        [&](int k) { return (k == 0 && !gz) ? nx : 0; },
        [&](int k, int c, double mine, double* lam_next) {
            if (c >= nx) a_[c - nx] += mine;                                // one lane per column and step; the step's barrier orders the steps
            else if (k > 0) lam_next[c] = mine;
            else gz[(size_t)b * nx + c] = (TIO)mine;
        },
        [&](int k, double* lam_next) {                                      // the accumulators keep what they hold
            for (int c = tid; c < nx; c += THREADS) {
                if (k > 0) lam_next[c] = 0.0;
                else if (gz) gz[(size_t)b * nx + c] = (TIO)0.0;
            }
        },
        [](int, double*) {});
    // the accumulators: rounded once per environment, and / or handed to the reduction over the batch as fp64
    TIO* const ge = DJ_GLOBAL_PTR(TIO, A.gtheta_env); double* const out = DJ_GLOBAL_PTR(double, A.acc_out);
    for (int e = tid; e < nth; e += THREADS) {
        if (ge) ge[(size_t)b * nth + e] = (TIO)a_[e];
        if (out) out[(size_t)b * nth + e] = a_[e];
    }
}

// gtheta[e] = sum_b acc[b][e]: workgroup e, lane t adds the environments t, t + 256, ...; then the tree
template <class TIO>
__global__ void __launch_bounds__(THREADS) data_reduce_kernel(const double* acc_, int B, int nth, TIO* gtheta_) {
    using namespace adjoint;
    __shared__ double rows_[TEAMS];
    const int e = (int)blockIdx.x, tid = (int)threadIdx.x;
    const double* const acc = DJ_GLOBAL_PTR(const double, acc_);
    double s = 0.0;
    for (int b = tid; b < B; b += THREADS) s += acc[(size_t)b * nth + e];
    s = row_sum(s);
    if (tid % ROW == 0) rows_[tid / ROW] = s;
    __syncthreads();
    if (tid < ROW) {                                                        // (TEAMS == ROW: the sixteen row sums fill one DPP row)
        s = row_sum(rows_[tid]);
        if (tid == 0) DJ_GLOBAL_PTR(TIO, gtheta_)[e] = (TIO)s;
    }
}
#endif

}  // namespace dadjoint
}  // namespace dj
