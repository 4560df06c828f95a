// dojo_adjoint.hpp -- reverse sweep over the recorded IFT Jacobians of a rollout (dojo_rollout_adjoint_dev; no counterpart in the reference,
// which differentiates one step at a time: src/gradients/state.jl:69-126).
//
// Per environment b, with g_k the cotangent of the loss w.r.t. the state after step k (tangent coordinates [x; v; phi; omega] per body):
//
//     lambda <- g_{H-1}
//     for k = H-1 .. 0:   failed step (status[k][b] != 0):  gU[k][b] <- 0,                    lambda <- 0      (by select: its Jacobians are never read)
//                         else:                             gU[k][b] <- DU_k[b]^T lambda,     lambda <- DZ_k[b]^T lambda
//                         if k > 0: lambda <- lambda + g_{k-1}
//     gz[b] <- lambda
//
// The Jacobians are in the device layout of dojo_step_dev: column-major per environment, DZ[k][b][c][r] = d x_{k+1}[r] / d x_k[c], so that a
// COLUMN is contiguous and (DZ^T lambda)[c] is the dot product of that column with lambda.  The job is H transposed mat-vecs over matrices that
// are read exactly once: HBM streaming with a serial dependency through lambda.
//
// Mapping: one workgroup of 256 lanes per environment, one launch for all H steps.  lambda lives in LDS as fp64, double-buffered, and so does the
// cotangent g_k that joins it (4 nx doubles in all; g_{k-1} is fetched while step k runs); one barrier per step.  Sixteen lanes (a DPP row) share a column: lane j of the row takes the 16-byte pieces j, j + 16, ... of it (nx = 12 Nb: every
// column starts 16-byte aligned and holds whole pieces in both dtypes), multiplies them in fp64 with its rows of lambda, and the row's sixteen
// partial sums meet in four DPP rotations.  A row keeps COLS columns in flight; the work of a step is a flat list of (column group, piece) items and
// the loads of item i + 1 are issued before the arithmetic of item i -- across the barrier too: the first loads of step k - 1 leave before step k ends.
// The summation order is fixed by (nx, dtype) alone: no atomics, results are bit-identical from run to run and do not depend on the batch size or on
// where in the batch an environment sits.
//
// What the other reverse sweeps take from here (dojo_data_adjoint.hpp, dojo_policy_adjoint.hpp, dojo_mlp.hpp): cotangent() and its record Cot, the column
// pipeline (columns, items, issue, consume) and sweep(), the loop over the steps that drives it -- the g buffers, the two piece buffers, which item
// is issued next across a step boundary, the failed steps, the barrier.  A kernel is its set-up, four callables for sweep() and its write-out.
#pragma once
#include <hip/hip_runtime.h>
#include "dojo_math.hpp"

namespace dj {
namespace adjoint {

// what cotangent() reads: the cotangents of the states of a rollout, in either space.  Every sweep builds one from its own argument record.
template <class TIO> struct Cot {
    const TIO* G;           // [H][B][nx] (cot_space 0) or [H][B][13 Nb] (cot_space 1)
    const TIO* Z;           // [H][B][13 Nb], cot_space 1 only
    int B, nx, cot_space;
};

template <class TIO> struct Args {
    const TIO* DZ;          // [H][B][nx][nx]
    const TIO* DU;          // [H][B][nu][nx] (unused when gU is null)
    const TIO* G;           // as Cot
    const TIO* Z;
    const int* status;      // [H][B] or null
    TIO* gU;                // [H][B][nu] or null
    TIO* gz;                // [B][nx] or null
    int H, B, nx, nu, cot_space;
};

constexpr int THREADS = 256, ROW = 16, COLS = 4, TEAMS = THREADS / ROW;     // lanes per workgroup, per column, columns in flight per row, rows
inline size_t lds_bytes(int nx) { return (size_t)4 * nx * sizeof(double); }     // lambda and g, double-buffered

#if defined(__HIPCC__)
template <class TIO> struct Piece;                                          // the 16 bytes a lane loads at once
template <> struct Piece<float>  { typedef float4 type;  static constexpr int N = 4; };
template <> struct Piece<double> { typedef double2 type; static constexpr int N = 2; };
__device__ __forceinline__ void unpack(const float4& v, double (&o)[4]) { o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w; }
__device__ __forceinline__ void unpack(const double2& v, double (&o)[2]) { o[0] = v.x; o[1] = v.y; }

template <int CTRL> __device__ __forceinline__ double dpp(double v) {
    return __hiloint2double(__builtin_amdgcn_mov_dpp(__double2hiint(v), CTRL, 0xF, 0xF, true), __builtin_amdgcn_mov_dpp(__double2loint(v), CTRL, 0xF, 0xF, true));
}
// sum over the 16 lanes of a DPP row; every lane ends with the same bits (each stage adds the two halves of a period, in either order)
__device__ __forceinline__ double row_sum(double v) {
    v += dpp<0x128>(v);     // row_ror:8
    v += dpp<0x124>(v);     // row_ror:4
    v += dpp<0x122>(v);     // row_ror:2
    v += dpp<0x121>(v);     // row_ror:1
    return v;
}

// g_k[c] of environment b in tangent coordinates.  cot_space 1: the cotangent is given w.r.t. the state (x, v, q, omega) and pulled back through
// dq = q (x) (0, phi) (dojo_math.hpp: LVᵀmat), i.e. g_phi = vector part of conj(q) (x) g_q; x, v, omega are copied.  A 4-byte state stands for
// q / |q| (as the step kernels read it).
template <class TIO, class A_> __device__ __forceinline__ Cot<TIO> cot_of(const A_& A) {      // from any record with these five fields
    return Cot<TIO>{DJ_GLOBAL_PTR(const TIO, A.G), DJ_GLOBAL_PTR(const TIO, A.Z), A.B, A.nx, A.cot_space};
}
template <class TIO> __device__ __forceinline__ double cotangent(const Cot<TIO>& A, int k, int b, int c) {
    const TIO* const G = A.G; const TIO* const Z = A.Z;
    const size_t kb = (size_t)k * A.B + b;
    if (A.cot_space == 0) return (double)G[kb * A.nx + c];
    const int body = c / 12, i = c % 12;
    const size_t o = (kb * (size_t)(A.nx / 12) + body) * 13;
    if (i < 6) return (double)G[o + i];
    if (i >= 9) return (double)G[o + i + 1];
    double q[4], g[4];
    for (int n = 0; n < 4; ++n) { q[n] = (double)Z[o + 6 + n]; g[n] = (double)G[o + 6 + n]; }
    if (sizeof(TIO) < sizeof(double)) {
        const double iq = 1.0 / sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
        for (int n = 0; n < 4; ++n) q[n] *= iq;
    }
    // conj(q) (x) g = (s gs + v.gv, s gv - gs v - v x gv)
    const int a = i - 6, a1 = (a + 1) % 3, a2 = (a + 2) % 3;
    return q[0] * g[1 + a] - g[0] * q[1 + a] - (q[1 + a1] * g[1 + a2] - q[1 + a2] * g[1 + a1]);
}

// ---- the column pipeline: what sweep() below streams DZ and DU with ----
// The columns of a step are [c0, nx) of DZ followed by ncol - nx columns of DU; its work is a flat list of (column group, piece) items.
template <class TIO> struct Columns {
    const TIO *DZ, *DU;     // the record (global address space)
    int B, nx, nu;          // nu: the columns of a DU block (the stride of the record, whether or not they are swept)
    int ncol, nM;           // nx + the DU columns that are swept; pieces of a column per lane
};
template <class TIO> __device__ __forceinline__ Columns<TIO> columns(const TIO* DZ, const TIO* DU, int B, int nx, int nu, int nu_swept) {
    return Columns<TIO>{DZ, DU, B, nx, nu, nx + nu_swept, (nx + ROW * Piece<TIO>::N - 1) / (ROW * Piece<TIO>::N)};
}
// items of a step whose columns start at c0 (an even number: the two piece buffers of a sweep take turns, and every step starts in the first; the odd one
// out is an item past the last group, whose lanes re-read one cached piece and write nothing)
template <class TIO> __device__ __forceinline__ int items(const Columns<TIO>& C, int c0) { return ((C.ncol - c0 + TEAMS * COLS - 1) / (TEAMS * COLS) * C.nM + 1) / 2 * 2; }
// loads of item `it` of step k of environment b: this lane's piece m of its row's COLS columns of group g.  Always COLS loads, so that the wait in front of
// the arithmetic can count them: a lane whose piece or column does not exist reads the first piece of the step's first column instead (and drops it).
template <class TIO> __device__ __forceinline__ void issue(const Columns<TIO>& C, int k, int b, int c0, int it, int team, int j, typename Piece<TIO>::type (&v)[COLS]) {
    typedef typename Piece<TIO>::type P;
    constexpr int V = Piece<TIO>::N;
    const int nx = C.nx, g = it / C.nM, m = it - g * C.nM, r0 = (m * ROW + j) * V, cb = c0 + g * TEAMS * COLS + team;
    const size_t kb = (size_t)k * C.B + b;
#pragma unroll
    for (int i = 0; i < COLS; ++i) {
        const bool ok = cb + i * TEAMS < C.ncol && r0 < nx;
        const int c = ok ? cb + i * TEAMS : c0, r = ok ? r0 : 0;
        const TIO* col = c < nx ? C.DZ + (kb * nx + c) * nx : C.DU + (kb * C.nu + (c - nx)) * nx;
        v[i] = *reinterpret_cast<const P*>(col + r);
    }
}
// arithmetic of item `it`: the loaded pieces times (lam + gk), accumulated per column; when the group's columns are complete the row's sixteen partial
// sums meet (row_sum) and lane i of the row hands column i to put(column, value)
template <class TIO, class Put>
__device__ __forceinline__ void consume(const Columns<TIO>& C, int c0, int it, int team, int j, const double* lam, const double* gk,
                                        const typename Piece<TIO>::type (&cur)[COLS], double (&acc)[COLS], Put&& put) {
    constexpr int V = Piece<TIO>::N;
    const int nx = C.nx, g = it / C.nM, m = it - g * C.nM, r0 = (m * ROW + j) * V;
    const bool have = r0 < nx;
    const int rl = have ? r0 : 0;
    double l[V];
#pragma unroll
    for (int n = 0; n < V; ++n) l[n] = lam[rl + n] + gk[rl + n];
#pragma unroll
    for (int i = 0; i < COLS; ++i) {
        double x[V]; unpack(cur[i], x);
#pragma unroll
        for (int n = 0; n < V; ++n) acc[i] = fma(have ? x[n] : 0.0, have ? l[n] : 0.0, acc[i]);
    }
    if (m == C.nM - 1) {                                                // the group's columns are complete: lane i of the row writes column i
        double mine = 0.0;
#pragma unroll
        for (int i = 0; i < COLS; ++i) { const double s_ = row_sum(acc[i]); if (j == i) mine = s_; acc[i] = 0.0; }
        const int c = c0 + g * TEAMS * COLS + team + j * TEAMS;
        if (j < COLS && c < C.ncol) put(c, mine);
    }
}

// ---- the step loop: what the four reverse sweeps (this one, dojo_data_adjoint.hpp, dojo_policy_adjoint.hpp, dojo_mlp.hpp) walk the record with ----
// Called by all 256 lanes of environment b's workgroup with lambda (what flows into step H-1 next to g_{H-1}; the open-loop sweeps: 0) in lam_[0 .. nx).
// It owns g_k in LDS (double-buffered; g_{k-1} is fetched through cotangent() while step k runs), the two piece buffers and which item is issued
// next, the failed steps (status != 0: no item is issued, nothing of DZ_k or DU_k is read) and the barrier that ends a step.  The kernel hands it
//     first_col(k)                     where the step's columns start (uniform over the workgroup)
//     put(k, c, value, lam_next)       a finished column c of step k: one lane per column
//     on_failed(k, lam_next)           what a failed step writes in their place: all lanes
//     after(k, lam_next)               behind the step's barrier, all lanes: uniform over the workgroup, may contain barriers of its own and must end
//                                      with one if it writes what the next step reads (lam_next is lambda of step k-1, less g_{k-1})
// lam_ [2][nx] and g_ [2][nx] are LDS.  Everything is inlined into the kernel: the callables cost no registers of their own.
template <class TIO, class FirstCol, class Put, class OnFailed, class After>
__device__ __forceinline__ void sweep(const Columns<TIO>& C, const Cot<TIO>& cot, const int* status, int H, int b, double* lam_, double* g_,
                                      FirstCol&& first_col, Put&& put, OnFailed&& on_failed, After&& after) {
    typedef typename Piece<TIO>::type P;
    const int tid = (int)threadIdx.x, team = tid / ROW, j = tid % ROW, B = C.B, nx = C.nx;
    auto failed = [&](int k) { return status != nullptr && status[(size_t)k * B + b] != 0; };
    auto items_of = [&](int k) { return (k < 0 || failed(k)) ? 0 : items(C, first_col(k)); };

    for (int c = tid; c < nx; c += THREADS) g_[((H - 1) & 1) * nx + c] = cotangent(cot, H - 1, b, c);
    // Two piece buffers take turns: a copy from "next" to "current" would have to wait for the loads it is meant to leave in flight.
    int p = 0, nit = items_of(H - 1);
    P buf0[COLS], buf1[COLS];
    if (nit) issue(C, H - 1, b, first_col(H - 1), 0, team, j, buf0);
    __syncthreads();
    for (int k = H - 1; k >= 0; --k) {
        // lambda_k = (what step k + 1 left) + g_k, formed where it is read; g_{k-1} goes to LDS for the next step meanwhile
        const double* lam = lam_ + p * nx; const double* gk = g_ + (k & 1) * nx; double* lam_next = lam_ + (p ^ 1) * nx;
        const int nit_next = items_of(k - 1), c0 = first_col(k);
        if (k > 0) for (int c = tid; c < nx; c += THREADS) g_[((k - 1) & 1) * nx + c] = cotangent(cot, k - 1, b, c);
        double acc[COLS];
#pragma unroll
        for (int i = 0; i < COLS; ++i) acc[i] = 0.0;
        auto put_k = [&](int c, double mine) { put(k, c, mine, lam_next); };
        auto stage = [&](int it, const P (&cur)[COLS], P (&nxt)[COLS]) {
            // the next item: of this step, else the first of step k - 1 -- else this one again, so that a wait always has COLS younger loads to count
            const bool more = it + 1 < nit;
            const int kn = (more || !nit_next) ? k : k - 1;
            issue(C, kn, b, first_col(kn), more ? it + 1 : nit_next ? 0 : it, team, j, nxt);
            consume(C, c0, it, team, j, lam, gk, cur, acc, put_k);
        };
        for (int it = 0; it < nit; it += 2) { stage(it, buf0, buf1); stage(it + 1, buf1, buf0); }
        if (failed(k)) {                                                    // nothing flows through a failed step
            on_failed(k, lam_next);
            if (nit_next) issue(C, k - 1, b, first_col(k - 1), 0, team, j, buf0);
        }
        __syncthreads();
        after(k, lam_next);
        p ^= 1; nit = nit_next;
    }
}

template <class TIO>
__global__ void __launch_bounds__(THREADS) rollout_adjoint_kernel(const Args<TIO> A) {
    extern __shared__ __align__(16) double lds_[];                          // lambda [2][nx] | g [2][nx]
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
    const int nx = A.nx, nu = A.gU ? A.nu : 0;
    TIO* const gU = DJ_GLOBAL_PTR(TIO, A.gU); TIO* const gz = DJ_GLOBAL_PTR(TIO, A.gz);
    const Columns<TIO> C = columns<TIO>(DJ_GLOBAL_PTR(const TIO, A.DZ), DJ_GLOBAL_PTR(const TIO, A.DU), A.B, nx, A.nu, nu);
    double* const lam_ = lds_;

    for (int c = tid; c < nx; c += THREADS) lam_[c] = 0.0;
    sweep(C, cot_of<TIO>(A), DJ_GLOBAL_PTR(const int, A.status), A.H, b, lam_, lds_ + 2 * nx,
        // the columns of step k: [c0, nx) of DZ (lambda; step 0 feeds gz alone), then the nu columns of DU (gU)
        [&](int k) { return (k == 0 && !gz) ? nx : 0; },
        [&](int k, int c, double mine, double* lam_next) {
            if (c >= nx) gU[((size_t)k * A.B + b) * A.nu + (c - nx)] = (TIO)mine;
            else if (k > 0) lam_next[c] = mine;
            else gz[(size_t)b * nx + c] = (TIO)mine;
        },
        [&](int k, double* lam_next) {
            for (int c = tid; c < nx; c += THREADS) {
                if (k > 0) lam_next[c] = 0.0;
                else if (gz) gz[(size_t)b * nx + c] = (TIO)0.0;
            }
            for (int c = tid; c < nu; c += THREADS) gU[((size_t)k * A.B + b) * A.nu + c] = (TIO)0.0;
        },
        [](int, double*) {});
}
#endif

}  // namespace adjoint
}  // namespace dj
