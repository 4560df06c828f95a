// dojo_policy.hpp -- the controller of a closed-loop rollout (dojo_rollout_policy_dev): observation, normalisation, affine policy and control
// assembly in ONE launch between two steps of an environment group.  The reference's counterpart is the `control!` callback of
// simulate!(mechanism, steps, storage, control!) (src/simulation/simulate.jl:16-37) with the policies of its examples: u = -K x
// (examples/control/cartpole_lqr.jl), a linear policy on normalised observations (examples/learning/ant_ars.jl:78-115).
//
// Per environment b and step k, with z_k the state the step starts from:
//
//     o_k   = [maximal_to_minimal(z_k) (2 nu);  clamp(gamma_c of step k - 1, -1, 1) per contact c (Nc, optional)]      rounded once to the ABI type, -> OBS[k][b]
//     ohat  = (o_k - mean) .* scale                                                                                    from the ROUNDED o_k, fp64
//     a_i   = bias_i + sum_j W[i][j] ohat_j                     i = 0 .. na - 1                                       fp64
//     u     = U_ff[k][b];  u[act_off + i] += a_i                                                                       rounded once, -> U_out[k][b], read by step k
//
// (the contact entries of o_0 are the neutral 1.0 of a fresh ContactConstraint unless the caller asks for the handle's last solution).  What is
// recorded is what the policy saw: U_out can be recomputed from OBS alone.
//
// Mapping: one wavefront per environment, four environments per 256-lane workgroup.  The work is tiny (the Ant of AntARS: 13 joint maps, 9 contacts, an 8 x 37
// mat-vec, 1.2 KB of W), so the goal is one launch without scratch memory and a short latency, not throughput.
//   Phase A  (observe(), shared with the network controller of dojo_mlp.hpp) lane l takes the joints l, l + 64, ...: coords::load_body +
//            coords::joint_max2min, the source max2min_kernel is made of; lanes take the contacts the way contact_obs_kernel does.  The rounded o goes to OBS (if given), ohat to LDS as fp64 ([4][nobs]).
//   barrier  (every wavefront of the workgroup reaches it: a wavefront whose environment does not exist does no work, but does not return before it)
//   Phase B  per action i: lane j accumulates W[i][j] ohat_j, W[i][j + 64] ohat_{j + 64}, ... with fma in ascending order (loads coalesced along nobs);
//            the 64 partial sums meet in a fixed order: four DPP row rotations inside every 16-lane row (adjoint::row_sum), then the four row sums
//            added in row order.  The lane (act_off + i) mod 64 stores u[act_off + i]; lanes c, c + 64, ... copy the inputs the policy does not drive.
// The summation order depends on nobs alone: no atomics, results are bit-identical from run to run and do not depend on the number of environment
// groups, on where in the batch an environment sits, or on whether W is shared (per_env = 0) or given per environment.
// An observation-only launch (u = null: OBS[H], the observation of the final state) ends after phase A.
#pragma once
#include <hip/hip_runtime.h>
#include "dojo_math.hpp"
#include "dojo_coords.hpp"
#include "dojo_adjoint.hpp"

namespace dj {
namespace policy {

template <class TIO> struct Args {
    const NodeP<double>* nodes;
    const TIO* z;                       // [B][13 Nb]: the state the step starts from
    const TIO* csg;                     // [B][8 Nc]: [s; gamma] per contact of the previous step; null = the neutral 1.0
    const TIO *W, *bias, *mean, *scale; // [Bw][na][nobs], [Bw][na] or null, [nobs] or null, [nobs] or null
    const TIO* uff;                     // [B][nu] of this step or null
    TIO* obs;                           // [B][nobs] of this step or null
    TIO* u;                             // [B][nu] of this step; null = observation only
    int env0, nenv;                     // the environments of this launch (all pointers are batch-level)
    int Nb, nu, Nc, nobs, act_off, na, per_env;
    double dt;
};

constexpr int THREADS = 256, WAVE = 64, ENVS = THREADS / WAVE;
inline size_t lds_bytes(int nobs) { return (size_t)ENVS * nobs * sizeof(double); }

#if defined(__HIPCC__)
__device__ __forceinline__ double lane_value(double v, int lane) {      // v of a given lane, in every lane
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane), __builtin_amdgcn_readlane(__double2loint(v), lane));
}
// sum over the 64 lanes of a wavefront in a fixed order: inside the rows as adjoint::row_sum, then the rows in row order
__device__ __forceinline__ double wave_sum(double v) {
    v = adjoint::row_sum(v);
    return ((lane_value(v, 0) + lane_value(v, 16)) + lane_value(v, 32)) + lane_value(v, 48);
}

// Phase A for one live wavefront, of this controller and of the network's (dojo_mlp.hpp; A: either argument record): o rounded to the ABI type goes to obs
// (if given) -- recorded, and what the policy consumes -- and (o - mean) .* scale to oh
template <class TIO, class A_>
__device__ __forceinline__ void observe(const A_& A, const NodeP<double>* nodes, const TIO* ze, const TIO* csg, const TIO* mean, const TIO* scale, size_t env, int lane,
                                        TIO* obs, double* oh) {
    using namespace coords;
    const int Nb = A.Nb, nu = A.nu, Nc = A.Nc;
    auto put = [&](int j, double v) {
        const TIO r = (TIO)v;
        if (obs) obs[j] = r;
        oh[j] = ((double)r - (mean ? (double)mean[j] : 0.0)) * (scale ? (double)scale[j] : 1.0);
    };
    for (int k = lane; k < Nb; k += WAVE) {
        const NodeP<double>& P = nodes[k];
        const int nt = P.nu_t, nr = P.nu_r, n = nt + nr, o = 2 * P.u_off;
        double ct[3], cr[3], vt[3], vr[3];
        const PoseVel<double> b = load_body<double>(ze, k), a = P.parent >= 0 ? load_body<double>(ze, P.parent) : origin_body<double>();
        joint_max2min(ct, cr, vt, vr, P, A.dt, a, b);
        for (int i = 0; i < 3; ++i) { if (i < nt) { put(o + i, ct[i]); put(o + n + i, vt[i]); } if (i < nr) { put(o + nt + i, cr[i]); put(o + n + nt + i, vr[i]); } }
    }
    for (int c = lane; c < Nc; c += WAVE) {
        const double g = csg ? (double)csg[env * 8 * Nc + 8 * c + 4] : 1.0;
        put(2 * nu + c, g < -1.0 ? -1.0 : g > 1.0 ? 1.0 : g);
    }
}

template <class TIO>
__global__ void __launch_bounds__(THREADS) rollout_policy_kernel(const Args<TIO> A) {
    extern __shared__ __align__(16) double lds_[];                          // ohat [ENVS][nobs]
    const int tid = (int)threadIdx.x, wave = tid / WAVE, lane = tid % WAVE;
    const int e = (int)blockIdx.x * ENVS + wave;
    const bool live = e < A.nenv;
    const size_t env = (size_t)A.env0 + (live ? e : 0);
    const int nu = A.nu, nobs = A.nobs;
    const NodeP<double>* const nodes = DJ_GLOBAL_PTR(const NodeP<double>, A.nodes);
    const TIO* const ze = DJ_GLOBAL_PTR(const TIO, A.z) + env * 13 * A.Nb;
    const TIO* const csg = DJ_GLOBAL_PTR(const TIO, A.csg);
    const TIO* const mean = DJ_GLOBAL_PTR(const TIO, A.mean); const TIO* const scale = DJ_GLOBAL_PTR(const TIO, A.scale);
    TIO* const obs = A.obs ? DJ_GLOBAL_PTR(TIO, A.obs) + env * nobs : nullptr;
    double* const oh = lds_ + wave * nobs;
    if (live) observe<TIO>(A, nodes, ze, csg, mean, scale, env, lane, obs, oh);
    if (!A.u) return;                                                       // (uniform over the launch)
    __syncthreads();
    if (!live) return;                                                      // (uniform over the wavefront: the DPP sums below see all 64 lanes)
    const TIO* const W = DJ_GLOBAL_PTR(const TIO, A.W) + (A.per_env ? env : (size_t)0) * A.na * nobs;
    const TIO* const bias = A.bias ? DJ_GLOBAL_PTR(const TIO, A.bias) + (A.per_env ? env : (size_t)0) * A.na : nullptr;
    const TIO* const uff = A.uff ? DJ_GLOBAL_PTR(const TIO, A.uff) + env * nu : nullptr;
    TIO* const u = DJ_GLOBAL_PTR(TIO, A.u) + env * nu;
    for (int c = lane; c < nu; c += WAVE)
        if (c < A.act_off || c >= A.act_off + A.na) u[c] = uff ? uff[c] : (TIO)0.0;
    for (int i = 0; i < A.na; ++i) {
        const TIO* const Wi = W + (size_t)i * nobs;
        double acc = 0.0;
        for (int j = lane; j < nobs; j += WAVE) acc = fma((double)Wi[j], oh[j], acc);
        const double a = (bias ? (double)bias[i] : 0.0) + wave_sum(acc);
        const int c = A.act_off + i;
        if (lane == c % WAVE) u[c] = (TIO)((uff ? (double)uff[c] : 0.0) + a);
    }
}
#endif

}  // namespace policy
}  // namespace dj
