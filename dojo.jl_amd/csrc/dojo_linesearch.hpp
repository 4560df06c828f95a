// dojo_linesearch.hpp -- the selection step of a side-by-side line search (dojo_linesearch_select_dev, include/dojo_hip_linesearch.h): the costs of the T trials
// of every problem, the Armijo test, the first acceptable trial, and the gather of its trajectory.  The reference's counterpart is the loop over the step
// lengths in IterativeLQR's forward pass; here the T trials exist already (the fan, dojo_rollout_minimal_fan_dev) and only the decision is left.
//
// Mapping: one 256-lane workgroup per problem p, wavefront w of its four takes the trials w, w + 4, ..; the trajectory the pass was taken around counts as
// trial T when its cost is wanted.  A trial's cost: lane j owns the rows j, j + 64, .. of every matrix-vector product (n = 72 takes two rounds), forms
// r = sum_c M[j][c] d_c and adds d_j r to its partial sum, all with fma in ascending order; the 64 partial sums meet once per trial in policy::wave_sum.  The
// matrices are shared by every problem and stay in cache; d_c is a wavefront-uniform address.  The T costs and flags meet in LDS (65 doubles, 64 ints) behind the
// kernel's one barrier; every lane runs the same ascending scan, so the choice is uniform without a broadcast; then all 256 lanes copy the chosen columns,
// consecutive lanes along n / nu.  No atomics; nothing depends on P or on the block index beyond the addresses: bit-identical from run to run, across P and
// across the place of a problem.
#pragma once
#include <hip/hip_runtime.h>
#include "dojo_policy.hpp"

namespace dj {
namespace linesearch {

constexpr int THREADS = 256, WAVE = 64, WAVES = THREADS / WAVE, MAX_T = 64;

template <class TIO> struct Args {
    const TIO *X, *U; const int* status;            // [H+1][B][n], [H][B][nu], [H][B] or null
    const TIO *alpha, *dV; const int* ok;           // [T][P], [P][2], [P] or null
    const TIO *Xcur, *Ucur;                         // [H+1][P][n], [H][P][nu]
    const double* J0;                               // [P]; null: computed (needs the cost)
    double *J_trial, *J_cur, *J_acc;                // [T][P]: written with a cost, read without; [P] or null; [P]
    int* choice; TIO* alpha_acc;                    // [P]
    TIO *X_new, *U_new;                             // [H+1][P][n], [H][P][nu]; each may be null
    const TIO *Q, *R, *Qf, *goal;                   // the cost (Q null: none); goal [n], or [P][n] with goal_per_problem
    double c1;
    int goal_per_problem, H, T, P, nu, act_off, na;
};

#if defined(__HIPCC__)
// this lane's part of  sum_k d_k' Q d_k + u_k' R u_k  +  d_H' Qf d_H  over one trajectory: x, u point at its step 0, xs and us are the distances between two steps
template <class TIO>
__device__ __forceinline__ double cost_partial(const Args<TIO>& A, const TIO* x, size_t xs, const TIO* u, size_t us, const TIO* g, int lane) {
    const int n = 2 * A.nu, na = A.na;
    double acc = 0.0;
    for (int k = 0; k <= A.H; ++k, x += xs) {
        const TIO* const M = k < A.H ? A.Q : A.Qf;
        for (int j = lane; j < n; j += WAVE) {
            const TIO* const Mj = M + (size_t)j * n;
            double r = 0.0;
            for (int c = 0; c < n; ++c) r = fma((double)Mj[c], (double)x[c] - (double)g[c], r);
            acc = fma((double)x[j] - (double)g[j], r, acc);
        }
        if (k == A.H) break;
        const TIO* const ua = u + (size_t)k * us + A.act_off;
        for (int i = lane; i < na; i += WAVE) {
            const TIO* const Ri = A.R + (size_t)i * na;
            double r = 0.0;
            for (int c = 0; c < na; ++c) r = fma((double)Ri[c], (double)ua[c], r);
            acc = fma((double)ua[i], r, acc);
        }
    }
    return acc;
}

template <class TIO>
__global__ void __launch_bounds__(THREADS) linesearch_select_kernel(const Args<TIO> A) {
    __shared__ double sJ[MAX_T + 1];       // the costs of the trials; [T]: J0
    __shared__ int sBad[MAX_T];            // != 0: a failed step in the trial
    const int tid = (int)threadIdx.x, wave = tid / WAVE, lane = tid % WAVE;
    const int p = (int)blockIdx.x, P = A.P, T = A.T, H = A.H, nu = A.nu, n = 2 * nu;
    const size_t B = (size_t)T * P;
    const bool have_cost = A.Q != nullptr;
    const TIO* const g = have_cost ? A.goal + (A.goal_per_problem ? (size_t)p * n : 0) : nullptr;
    // trial T stands for the current trajectory (its cost alone, and only when it is not given)
    for (int tr = wave; tr <= T; tr += WAVES) {          // (uniform over the wavefront: wave_sum sees all 64 lanes)
        if (tr == T) {
            if (A.J0) { if (lane == 0) sJ[T] = A.J0[p]; }
            else {
                const double J = 0.5 * policy::wave_sum(cost_partial(A, A.Xcur + (size_t)p * n, (size_t)P * n, A.Ucur + (size_t)p * nu, (size_t)P * nu, g, lane));
                if (lane == 0) sJ[T] = J;
            }
            continue;
        }
        const size_t e = (size_t)tr * P + p;
        double J;
        if (have_cost) {
            J = 0.5 * policy::wave_sum(cost_partial(A, A.X + e * n, B * n, A.U + e * nu, B * nu, g, lane));
            if (lane == 0) A.J_trial[e] = J;
        }
        else J = A.J_trial[e];
        int bad = 0;
        if (A.status) for (int k = lane; k < H; k += WAVE) bad |= A.status[(size_t)k * B + e] != 0;
        bad = __any(bad);
        if (lane == 0) { sJ[tr] = J; sBad[tr] = bad; }
    }
    __syncthreads();
    const double J0 = sJ[T], dV0 = (double)A.dV[2 * (size_t)p], dV1 = (double)A.dV[2 * (size_t)p + 1];
    int choice = -1;
    if (!A.ok || A.ok[p] != 0)
        for (int tr = 0; tr < T; ++tr) {
            const double a = (double)A.alpha[(size_t)tr * P + p], J = sJ[tr];
            if (!sBad[tr] && J <= J0 + A.c1 * (a * dV0 + a * a * dV1)) { choice = tr; break; }      // (a NaN cost compares false)
        }
    if (tid == 0) {
        A.choice[p] = choice;
        A.alpha_acc[p] = choice >= 0 ? A.alpha[(size_t)choice * P + p] : (TIO)0.0;
        A.J_acc[p] = choice >= 0 ? sJ[choice] : J0;
        if (A.J_cur) A.J_cur[p] = J0;
    }
    // the gather: step k of the chosen trial, or of the current trajectory
    const size_t src = choice >= 0 ? (size_t)choice * P + p : (size_t)p, sB = choice >= 0 ? B : (size_t)P;
    if (A.X_new) {
        const TIO* const from = choice >= 0 ? A.X : A.Xcur;
        for (int i = tid; i < (H + 1) * n; i += THREADS) { const int k = i / n, c = i % n; A.X_new[((size_t)k * P + p) * n + c] = from[((size_t)k * sB + src) * n + c]; }
    }
    if (A.U_new) {
        const TIO* const from = choice >= 0 ? A.U : A.Ucur;
        for (int i = tid; i < H * nu; i += THREADS) { const int k = i / nu, c = i % nu; A.U_new[((size_t)k * P + p) * nu + c] = from[((size_t)k * sB + src) * nu + c]; }
    }
}
#endif

}  // namespace linesearch
}  // namespace dj
