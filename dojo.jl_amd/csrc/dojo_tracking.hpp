// dojo_tracking.hpp -- the control law of a rollout in minimal coordinates (dojo_rollout_minimal_dev, include/dojo_hip_trajopt.h): time-varying feedback around
// a reference trajectory, evaluated between two steps of an environment group.  The reference's counterpart is DojoEnvironments.step! (minimal state in, minimal
// state out: src/simulation/step.jl:42-60) under simulate! with a finite-horizon LQR / tracking controller, and the forward pass of IterativeLQR.
//
// Per environment b and step k, n = 2 nu, X[k] the minimal state in the ABI type (maximal_to_minimal of the state step k - 1 left; k = 0: x0):
//
//     dx_j  = (double)X[k][j] - (double)Xbar[k][b][j]                                           from the ROUNDED X[k], fp64
//     a_i   = fma(alpha[b], kff[k][b][i], sum_j K[k][b][i][j] dx_j)      i = 0 .. na - 1        fp64
//     u     = Ubar[k][b];  u[act_off + i] += a_i                                                rounded once, -> U_out[k][b], read by step k
//
// The two coordinate maps around it -- X[k] from the state the previous step left, and the maximal state step k starts from, re-projected from the rounded X[k] --
// are max2min_kernel and min2max_kernel of dojo_coord_kernels.hpp, launched by the host on the group's environments and stream in front of and behind this kernel.
// They were fused into this kernel at first (policy::observe in front, the root -> leaves walk of min2max_kernel by lane 0 behind: 190 VGPRs, no scratch); on the
// GPU that kernel's states differed from the two kernels' in the last bit on 68 of 81 920 environment-steps of the Ant (other fused multiply-add contractions in
// rarely taken branches of the joint maps), and the requirement is the bits of dojo_step_minimal_dev, so the maps stay the kernels that entry runs.
//
// Mapping: that of rollout_policy_kernel's phase B (dojo_policy.hpp) -- one wavefront per environment, four environments per 256-lane workgroup; per driven input i
// lane j accumulates K[i][j] dx_j, K[i][j + 64] dx_{j + 64}, ... with fma in ascending order (loads coalesced along n), the 64 partial sums meet in
// policy::wave_sum; lane (act_off + i) mod 64 stores u[act_off + i]; lanes c, c + 64, ... copy the inputs that are not driven.  No LDS, no barrier.
// No atomics; the summation order depends on n alone: results are bit-identical from run to run and do not depend on the environment groups or on where in the
// batch an environment sits.
#pragma once
#include <hip/hip_runtime.h>
#include "dojo_policy.hpp"
#include <type_traits>

namespace dj {
namespace tracking {

template <class TIO> struct Args {
    const TIO* X;                       // [B][n] of this step
    const TIO *ubar, *xbar, *K, *kff;   // of this step: [B][nu], [B][n], [B][na][n], [B][na]; each may be null
    const TIO* alpha;                   // [B] or null
    TIO* u;                             // [B][nu] of this step
    int env0, nenv;                     // the environments of this launch (all pointers are batch-level)
    int nu, act_off, na;
};

// the argument record of the clamped law (dojo_rollout_minimal_box_dev, include/dojo_hip_limits.h): rollout_tracking_kernel<TIO, BoxArgs<TIO>>
template <class TIO> struct BoxArgs : Args<TIO> {
    const TIO *lo, *hi;                 // [B][na] (batch-level); either may be null
};

// the argument record of the fan (dojo_rollout_minimal_fan_dev, include/dojo_hip_linesearch.h): rollout_tracking_kernel<TIO, FanArgs<TIO>>.  The batch is T trials
// of P problems, environment e = tr P + p: the reference members ubar, xbar, K, kff, lo, hi are [P][..] (the step's rows, P per step) and are read at p = e mod P;
// X, alpha and u stay per environment.  The law is the clamped one; with lo = hi = null it rounds the same fp64 sum as the plain one.
template <class TIO> struct FanArgs : BoxArgs<TIO> {
    int P;
};

#if defined(__HIPCC__)
// A_ = BoxArgs<TIO>: the clamped law (BOX; every difference sits behind `if constexpr (BOX)`: the instantiations over Args<TIO> keep their instructions)
// A_ = FanArgs<TIO>: the clamped law with the reference members read at e mod P (FAN; behind `if constexpr (FAN)`: the four other instantiations keep theirs)
template <class TIO, class A_ = Args<TIO>>
__global__ void __launch_bounds__(policy::THREADS) rollout_tracking_kernel(const A_ A) {
    constexpr bool FAN = std::is_same<A_, FanArgs<TIO>>::value, BOX = FAN || std::is_same<A_, BoxArgs<TIO>>::value;
    using policy::WAVE;
    const int tid = (int)threadIdx.x, wave = tid / WAVE, lane = tid % WAVE;
    const int e = (int)blockIdx.x * policy::ENVS + wave;
    if (e >= A.nenv) return;                                                // (uniform over the wavefront: the DPP sums below see all 64 lanes)
    const size_t env = (size_t)A.env0 + e;
    size_t ref = env;                                                       // where the reference members are read
    if constexpr (FAN) ref = (unsigned)(A.env0 + e) % (unsigned)A.P;                // (env0 + e < B fits an int: a 32-bit remainder, not the 64-bit software one)
    const int nu = A.nu, n = 2 * nu;
    const TIO* const x = DJ_GLOBAL_PTR(const TIO, A.X) + env * n;
    const TIO* const ubar = A.ubar ? DJ_GLOBAL_PTR(const TIO, A.ubar) + ref * nu : nullptr;
    const TIO* const xbar = (A.xbar && A.K) ? DJ_GLOBAL_PTR(const TIO, A.xbar) + ref * n : nullptr;
    const TIO* const K = A.K ? DJ_GLOBAL_PTR(const TIO, A.K) + ref * A.na * n : nullptr;
    const TIO* const kff = A.kff ? DJ_GLOBAL_PTR(const TIO, A.kff) + ref * A.na : nullptr;
    const double alpha = A.alpha ? (double)DJ_GLOBAL_PTR(const TIO, A.alpha)[env] : 1.0;
    TIO* const u = DJ_GLOBAL_PTR(TIO, A.u) + env * nu;
    for (int c = lane; c < nu; c += WAVE)
        if (c < A.act_off || c >= A.act_off + A.na) u[c] = ubar ? ubar[c] : (TIO)0.0;
    for (int i = 0; i < A.na; ++i) {
        double s = 0.0;
        if (K) {
            const TIO* const Ki = K + (size_t)i * n;
            double acc = 0.0;
            for (int j = lane; j < n; j += WAVE) acc = fma((double)Ki[j], (double)x[j] - (xbar ? (double)xbar[j] : 0.0), acc);
            s = policy::wave_sum(acc);
        }
        const double a = fma(alpha, kff ? (double)kff[i] : 0.0, s);
        const int c = A.act_off + i;
        if constexpr (BOX) {
            // min(max(Ubar + a, lo), hi) in fp64, rounded once.  The limits are values of the ABI type and rounding is monotone: clamping in front of the rounding
            // gives the bits of clamping behind it, and a driven input is inside [lo, hi] exactly
            double v = (ubar ? (double)ubar[c] : 0.0) + a;
            if (A.lo) { const double l = (double)DJ_GLOBAL_PTR(const TIO, A.lo)[ref * A.na + i]; v = v < l ? l : v; }
            if (A.hi) { const double h = (double)DJ_GLOBAL_PTR(const TIO, A.hi)[ref * A.na + i]; v = v > h ? h : v; }
            if (lane == c % WAVE) u[c] = (TIO)v;
        } else {
            if (lane == c % WAVE) u[c] = (TIO)((ubar ? (double)ubar[c] : 0.0) + a);
        }
    }
}
#endif

}  // namespace tracking
}  // namespace dj
