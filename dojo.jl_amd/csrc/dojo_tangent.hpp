// dojo_tangent.hpp -- forward sweep over the recorded IFT Jacobians of a rollout, T tangent directions at once (dojo_rollout_tangent_dev).  The reference
// chains the same products on the host, one step and one direction block at a time (examples/system_identification/utilities.jl:42-90).
//
// Per environment b and tangent t, with delta the tangent of the state (tangent coordinates [x; v; phi; omega] per body):
//
//     delta <- dz0[b][t]                         (0 when dz0 is NULL)
//     for k = 0 .. H-1:   failed step (status[k][b] != 0):  delta <- 0                                              (DZ_k, DU_k, DC_k are never loaded)
//                         else:                             delta <- DZ_k[b] delta + DU_k[b] dU[k][b][t] + DC_k[b] dtheta[t]
//                         dZ[k][b][t] <- delta
//
// This is the transpose of the rule of the reverse sweeps (dojo_adjoint.hpp, dojo_data_adjoint.hpp): nothing flows through a failed step, the tangent of the
// state after it is 0, later controls act again.
//
// The record is column-major per environment (DZ[k][b][c][r], a column is contiguous), so DZ delta is a LINEAR COMBINATION OF COLUMNS -- not the dot product
// per column that the column pipeline of dojo_adjoint.hpp computes.  Mapping chosen: teams over column subsets, lanes over rows.
//   * One workgroup of 256 lanes per (environment, chunk of NT = 4 tangents); the chunks are in the grid (blockIdx.x = b * ceil(T / NT) + chunk), one launch
//     for all H steps.  Every chunk reads the record for itself: T = 8 costs two passes (an order of the workgroups that puts the chunks of an environment on one
//     accelerator die, to share its L2, measured the same).
//   * A column of nx scalars is np = nx / V 16-byte pieces (V = 4 fp32 or 2 fp64 per piece).  A TEAM is np consecutive lanes: lane j of it owns the rows
//     j V .. j V + V - 1 for the whole sweep and keeps NT x V fp64 accumulators in registers across the column loop of a step.  There are
//     nteams = min(256 / np, 16) teams (Ant fp32: 6 teams of 39 lanes, Atlas fp32: 2 of 93, Atlas fp64: 1 of 186; lanes past the last team idle); team m takes
//     the columns m, m + nteams, ... of each block (DZ, then DU, then DC) in ascending order.  Consecutive teams read consecutive columns, consecutive lanes
//     consecutive pieces: a workgroup's loads of an item are one contiguous run of the record.
//   * Every loaded piece is multiplied into the NT tangents of the chunk: the inputs of the step x = [delta; dU_k; dtheta] sit in LDS as fp64, tangent index
//     fastest (x[c][NT]: the NT values of a column are 32 contiguous bytes, the same address for all lanes of a team -- a broadcast).
//   * The partial sums of the teams meet in LDS: red[team][NT][nx] fp64, added in ascending team order by the lane that then owns (t, r).  Because a team is a
//     whole column wide there are at most 256 V / nx of them: the buffer is <= 256 V NT doubles (32 KB fp32, 16 KB fp64) whatever nx is -- Atlas, where sixteen
//     teams' worth of [NT][nx] would not fit, has two.  Two barriers per step: partial sums complete | delta_k (and dU_{k+1}) in place.
//   * The work of a step is a flat list of items (COLS = 4 column groups each); the loads of item i + 1 are issued before the arithmetic of item i, across the
//     barriers too (the first item of step k + 1 leaves before step k's reduction), with two piece buffers taking turns as in dojo_adjoint.hpp.
//   * delta stays fp64 in LDS between the steps, every product and sum is fp64, outputs are rounded once.  No atomics.  The order of the additions is fixed by
//     (nx, nu, 5Nc, dtype) alone: which team owns a column depends on the column's index inside its block and on nteams; a chunk's slots are computed
//     independently of each other, a padded slot (t >= T) does the same operations on zeros, an absent input block (NULL dU / dtheta) is skipped, which adds
//     nothing to the same sums.  Results are bit-identical from run to run and do not depend on B, on where the environment sits in the batch, on T or on where
//     the tangent sits among the T.
//   * tan_space 1: the output is the push-forward to the state per body -- x, v, omega copied, dq = q (x) (0, phi) (dojo_math.hpp: LVᵀmat) with q from Z[k][b]
//     (a 4-byte state stands for q / |q|): the transpose of adjoint::cotangent for cot_space 1.  Z of a failed step is not read.
//
// Resources (hipcc -O3, gfx950; no scratch, no spills in either):  rollout_tangent_kernel<float>: 195 VGPRs, two workgroups per CU;  rollout_tangent_kernel<double>:
// 146 VGPRs, three.  (Launch bounds that ask for a third / fourth workgroup make the allocator spill -- 108 / 276 B of scratch in fp32 -- and are not used.)
// LDS (dynamic) = 8 NT ((nx + nu + 5Nc) + nteams nx) bytes:  Ant (nx 156, nu 14, 5Nc 20) fp32 36 032 B, fp64 21 056 B;  Atlas (nx 372, nu 36, 5Nc 100) fp32 40 064 B,
// fp64 28 160 B.  Measured (Ant fp32, B 4096, H 20, tools/tangent_bench.py): T = 1 0.116 ms per step (3.8 TB/s of DZ + DU), T = 4 0.123, T = 8 0.206.
#pragma once
#include <hip/hip_runtime.h>
#include "dojo_math.hpp"
#include "dojo_adjoint.hpp"

namespace dj {
namespace tangent {

template <class TIO> struct Args {
    const TIO* DZ;          // [H][B][nx][nx]
    const TIO* DU;          // [H][B][nu][nx] (unused when dU is null)
    const TIO* DC;          // [H][B][nth][nx] (unused when dth is null)
    const TIO* dz0;         // [B][T][nx] or null
    const TIO* dU;          // [H][B][T][nu] or null
    const TIO* dth;         // [T][nth] or null
    const TIO* Z;           // [H][B][13 Nb], tan_space 1 only
    const int* status;      // [H][B] or null
    TIO* dZ;                // [H][B][T][nx] (tan_space 0) or [H][B][T][13 Nb] (tan_space 1)
    int H, B, T, nx, nu, nth, tan_space;
};

constexpr int THREADS = 256, NT = 4, COLS = 4, MAX_TEAMS = 16;      // lanes per workgroup, tangents per chunk, column groups in flight per lane, teams at most
inline int pieces(int nx, size_t w) { return (int)((size_t)nx * w / 16); }                                         // 16-byte pieces of a column = lanes of a team
inline int teams(int nx, size_t w) { const int t = THREADS / pieces(nx, w); return t < MAX_TEAMS ? t : MAX_TEAMS; }
inline bool fits(int nx, size_t w) { return pieces(nx, w) <= THREADS; }
inline size_t lds_bytes(int nx, int nu, int nth, size_t w) { return ((size_t)(nx + nu + nth) + (size_t)teams(nx, w) * nx) * NT * sizeof(double); }     // x | red

#if defined(__HIPCC__)
template <class TIO>
__global__ void __launch_bounds__(THREADS) rollout_tangent_kernel(const Args<TIO> A) {
    using adjoint::Piece; using adjoint::unpack;
    typedef typename Piece<TIO>::type P;
    constexpr int V = Piece<TIO>::N;
    extern __shared__ __align__(16) double lds_[];                          // x [nx + nu + nth][NT] | red [nteams][NT][nx]
    const int H = A.H, B = A.B, T = A.T, nx = A.nx, nu = A.dU ? A.nu : 0, nth = A.dth ? A.nth : 0, nchunk = (T + NT - 1) / NT;
    const int b = (int)blockIdx.x / nchunk, t0 = ((int)blockIdx.x - b * nchunk) * NT, tid = (int)threadIdx.x;
    const int np = nx / V, nteams = THREADS / np < MAX_TEAMS ? THREADS / np : MAX_TEAMS, team = tid / np, r0 = (tid - team * np) * V;
    const bool lane = team < nteams;                                        // (the lanes behind the last team load a piece they drop and add zeros)
    const int G = nteams * COLS, gz = (nx + G - 1) / G, gu = (nu + G - 1) / G, gc = (nth + G - 1) / G;
    const int nit_step = (gz + gu + gc + 1) / 2 * 2;                        // an even number: the two piece buffers take turns and every step starts in the first
    const TIO* const DZ = DJ_GLOBAL_PTR(const TIO, A.DZ); const TIO* const DU = DJ_GLOBAL_PTR(const TIO, A.DU); const TIO* const DC = DJ_GLOBAL_PTR(const TIO, A.DC);
    const TIO* const dz0 = DJ_GLOBAL_PTR(const TIO, A.dz0); const TIO* const dU = DJ_GLOBAL_PTR(const TIO, A.dU); const TIO* const dth = DJ_GLOBAL_PTR(const TIO, A.dth);
    const TIO* const Z = DJ_GLOBAL_PTR(const TIO, A.Z); const int* const status = DJ_GLOBAL_PTR(const int, A.status);
    TIO* const dZ = DJ_GLOBAL_PTR(TIO, A.dZ);
    double* const x_ = lds_; double* const red_ = lds_ + (size_t)(nx + nu + nth) * NT;

    auto failed = [&](int k) { return status != nullptr && status[(size_t)k * B + b] != 0; };
    auto items_of = [&](int k) { return (k >= H || failed(k)) ? 0 : nit_step; };
    // item `it` of a step: column group g of the block of n columns at `base` (the record of step kb), whose inputs start at x[xo]; past the last: n = 0
    auto locate = [&](size_t kb, int it, const TIO*& base, int& n, int& g, int& xo) {
        base = DZ + kb * nx * nx; n = nx; g = it; xo = 0;
        if (it >= gz) {
            g = it - gz;
            if (g < gu) { base = DU + kb * nu * nx; n = nu; xo = nx; }
            else { g -= gu; xo = nx + nu; if (g < gc) { base = DC + kb * nth * nx; n = nth; } else n = 0; }
        }
    };
    // loads of item `it` of step k: this lane's piece of its team's COLS columns.  Always COLS loads, so that the wait in front of the arithmetic can count
    // them: a lane whose column does not exist reads the first piece of the step's DZ instead (and drops it).
    auto issue = [&](int k, int it, P (&v)[COLS]) {
        const size_t kb = (size_t)k * B + b;
        const TIO* base; int n, g, xo; locate(kb, it, base, n, g, xo);
#pragma unroll
        for (int q = 0; q < COLS; ++q) {
            const int c = (g * COLS + q) * nteams + team;
            const bool ok = lane && c < n;
            v[q] = *reinterpret_cast<const P*>(ok ? base + (size_t)c * nx + r0 : DZ + kb * nx * nx);
        }
    };
    // arithmetic of item `it`: every loaded piece times the NT inputs of its column, into the lane's NT x V accumulators
    auto consume = [&](int it, const P (&cur)[COLS], double (&acc)[NT][V]) {
        const TIO* base; int n, g, xo; locate(0, it, base, n, g, xo);
#pragma unroll
        for (int q = 0; q < COLS; ++q) {
            const int c = (g * COLS + q) * nteams + team;
            const bool ok = lane && c < n;
            const double* xc = x_ + (size_t)(ok ? xo + c : 0) * NT;
            double m[V]; unpack(cur[q], m);
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const double xv = ok ? xc[t] : 0.0;
#pragma unroll
                for (int i = 0; i < V; ++i) acc[t][i] = fma(ok ? m[i] : 0.0, xv, acc[t][i]);
            }
        }
    };

    // the inputs of step 0: delta = dz0, dU_0, dtheta (the tangents past T: zeros)
    for (int e = tid; e < NT * nx; e += THREADS) {
        const int t = e / nx, r = e - t * nx;
        x_[r * NT + t] = (dz0 && t0 + t < T) ? (double)dz0[((size_t)b * T + t0 + t) * nx + r] : 0.0;
    }
    for (int e = tid; e < NT * nu; e += THREADS) {
        const int t = e / nu, c = e - t * nu;
        x_[(nx + c) * NT + t] = t0 + t < T ? (double)dU[((size_t)b * T + t0 + t) * nu + c] : 0.0;
    }
    for (int e = tid; e < NT * nth; e += THREADS) {
        const int t = e / nth, c = e - t * nth;
        x_[(nx + nu + c) * NT + t] = t0 + t < T ? (double)dth[(size_t)(t0 + t) * nth + c] : 0.0;
    }
    const int ut = nu ? tid / nu : NT, uc = nu ? tid - ut * nu : 0;      // the element of dU_{k+1} this lane fetches while step k runs (NT nu <= 256; the rest: below)
    int nit = items_of(0);
    P buf0[COLS], buf1[COLS];
    if (nit) issue(0, 0, buf0);
    __syncthreads();
    for (int k = 0; k < H; ++k) {
        const int nit_next = items_of(k + 1);
        const size_t kb = (size_t)k * B + b;
        const bool f = nit == 0;                                            // failed(k)
        const bool ufetch = k + 1 < H && ut < NT && t0 + ut < T;
        const TIO unext = ufetch ? dU[((kb + B) * T + t0 + ut) * nu + uc] : (TIO)0;
        double acc[NT][V];
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int i = 0; i < V; ++i) acc[t][i] = 0.0;
        auto stage = [&](int it, const P (&cur)[COLS], P (&nxt)[COLS]) {
            // the next item: of this step, else the first of step k + 1 -- else this one again, so that a wait always has COLS younger loads to count
            const bool more = it + 1 < nit;
            issue((more || !nit_next) ? k : k + 1, more ? it + 1 : nit_next ? 0 : it, nxt);
            consume(it, cur, acc);
        };
        for (int it = 0; it < nit; it += 2) { stage(it, buf0, buf1); stage(it + 1, buf1, buf0); }
        if (f) { if (nit_next) issue(k + 1, 0, buf0); }                     // nothing flows through a failed step
        else if (lane) {
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int i = 0; i < V; ++i) red_[((size_t)team * NT + t) * nx + r0 + i] = acc[t][i];
        }
        __syncthreads();
        // delta_k[t][r]: the teams' partial sums in ascending team order; rounded once into the output
        for (int e = tid; e < NT * nx; e += THREADS) {
            const int t = e / nx, r = e - t * nx;
            double s = 0.0;
            if (!f) {
                s = red_[(size_t)t * nx + r];
                for (int m = 1; m < nteams; ++m) s += red_[((size_t)m * NT + t) * nx + r];
            }
            x_[r * NT + t] = s;
            if (A.tan_space == 0 && t0 + t < T) dZ[(kb * T + t0 + t) * nx + r] = (TIO)s;
        }
        if (k + 1 < H) {                                                    // dU_{k+1} joins it
            if (ut < NT) x_[(nx + uc) * NT + ut] = (double)unext;
            for (int e = tid + THREADS; e < NT * nu; e += THREADS) {
                const int t = e / nu, c = e - t * nu;
                x_[(nx + c) * NT + t] = t0 + t < T ? (double)dU[((kb + B) * T + t0 + t) * nu + c] : 0.0;
            }
        }
        __syncthreads();
        if (A.tan_space == 1) {                                             // the push-forward of delta_k to the state, per body
            const int nz = nx / 12 * 13;
            for (int e = tid; e < NT * nz; e += THREADS) {
                const int t = e / nz, o = e - t * nz, body = o / 13, i = o - body * 13;
                if (t0 + t >= T) continue;
                const double* d = x_ + (size_t)body * 12 * NT + t;         // d[i NT]: entry i of the body's tangent
                double val = 0.0;
                if (i < 6) val = d[i * NT];
                else if (i >= 10) val = d[(i - 1) * NT];
                else if (!f) {
                    const size_t zo = (kb * (size_t)(nx / 12) + body) * 13 + 6;
                    double q[4];
                    for (int n = 0; n < 4; ++n) q[n] = (double)Z[zo + n];
                    if (sizeof(TIO) < sizeof(double)) {
                        const double iq = 1.0 / sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
                        for (int n = 0; n < 4; ++n) q[n] *= iq;
                    }
                    // q (x) (0, phi) = (-v.phi, s phi + v x phi)
                    const double ph[3] = {d[6 * NT], d[7 * NT], d[8 * NT]};
                    if (i == 6) val = -(q[1] * ph[0] + q[2] * ph[1] + q[3] * ph[2]);
                    else { const int a = i - 7, a1 = (a + 1) % 3, a2 = (a + 2) % 3; val = q[0] * ph[a] + (q[1 + a1] * ph[a2] - q[1 + a2] * ph[a1]); }
                }
                dZ[(kb * T + t0 + t) * nz + o] = (TIO)val;
            }
        }
        nit = nit_next;
    }
}
#endif

}  // namespace tangent
}  // namespace dj
