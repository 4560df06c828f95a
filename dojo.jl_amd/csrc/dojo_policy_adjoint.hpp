// dojo_policy_adjoint.hpp -- reverse mode through a closed-loop rollout (dojo_rollout_policy_adjoint_dev): the gradient of a trajectory loss w.r.t. the
// affine feedback policy of dojo_policy.hpp, its feed-forward term and the initial state.  No counterpart in the reference, which differentiates one
// step at a time (src/gradients/state.jl:69-126); the observation Jacobian is maximal_to_minimal_jacobian (src/gradients/state.jl:9-56).
//
// Per environment b: z_0 = z0, z_k = Z[k-1]; o_k the minimal-coordinate observation of z_k; ohat_k = (o_k - mean) .* scale from the RECORDED, rounded
// OBS[k] (as the forward kernel forms it); u_k = U_ff[k] + E (bias + W ohat_k); M_k = d o_k / d z_k [2nu x nx] in the tangent coordinates
// [x; v; phi; omega] per body.  With the cotangents g_k (state after step k), GU_k (U_out[k]) and GO_k (OBS[k], k = 0 .. H):
//
//     lambda <- g_{H-1} + M_H^T GO_H;   gW <- 0;  gbias <- 0
//     for k = H-1 .. 0:   failed step (status[k][b] != 0):  lambda <- 0       (by select: DZ_k, DU_k are never read)
//                         gu     = DU_k^T lambda + GU_k                        -> gU[k]  (w.r.t. U_ff[k], all nu entries)
//                         a      = gu[act_off .. act_off + na - 1]
//                         gbias += a;   gW += a ohat_k^T
//                         go     = scale .* (W^T a) + GO_k
//                         lambda = DZ_k^T lambda + M_k^T go   (+ g_{k-1} if k > 0)
//     gz <- lambda
//
// mean and scale are frozen (no gradient), and the rounding of o_k is not differentiated.
//
// Three kernels.
//   observation_jacobian_kernel  M in COMPACT form, [n][B][2nu][24] fp64: row i is minimal coordinate i (the order of dojo_maximal_to_minimal), columns
//       0..11 the derivative w.r.t. the tangent coordinates of the PARENT body of the joint that owns the row, 12..23 w.r.t. its CHILD body.  One thread
//       per (state, environment, joint): the Dual<24> evaluation of coords::joint_max2min that max2min_jac_kernel is made of, rows placed where
//       rollout_policy_kernel::put places the observation.  It is off the serial chain of the sweep, so its register cost is paid once.
//   rollout_policy_adjoint_kernel  one workgroup of 256 lanes per environment, one launch for all H steps.  DZ and DU go through the column pipeline of
//       dojo_adjoint.hpp (adjoint::issue / adjoint::consume: 16-byte loads, two register buffers that take turns, row_sum, the next item in flight across
//       the barriers); gu lands in LDS as fp64.  Two short phases follow per step, each behind a barrier:
//         (i)  lanes c < nu round gu to gU; lanes j < nobs form go_j = scale_j sum_i W[i][j] a_i + GO_j (i ascending, W read coalesced along nobs); the
//              na nobs + na accumulators of gW / gbias live in LDS as fp64, entry e owned by lane e mod 256 (no races); ohat_k is in LDS, formed from the
//              recorded OBS[k] one phase earlier.
//         (ii) lanes over the columns c < nx add sum_r M[r][.] go_r to lam_next[c], r over the rows that touch body c / 12 -- its own joint's rows (child
//              half) and those of every joint whose parent it is -- in the ascending order of a CSR table (row, half) per body that the host builds once;
//              ohat_{k-1} goes to LDS.
//       LDS: lambda and g double-buffered (4 nx), gu (nu), go and ohat (2 nobs), the accumulators (na (nobs + 1)) doubles: Ant 7 KB, Atlas 30 KB.
//       All arithmetic is fp64, outputs are rounded once, no atomics: the summation order is fixed by (nx, nu, na, nobs, topology, dtype) alone.
//   policy_reduce_kernel  shared policy (per_env = 0): the sweep leaves the per-environment accumulators as fp64 in a workspace [B][na (nobs + 1)]; sixteen
//       lanes (a DPP row) share an entry, lane j adds the environments j, j + 16, ... in ascending order and the sixteen sums meet in adjoint::row_sum:
//       an order fixed by B alone.  Rounded once.
#pragma once
#include <hip/hip_runtime.h>
#include "dojo_math.hpp"
#include "dojo_coords.hpp"
#include "dojo_adjoint.hpp"

namespace dj {
namespace padjoint {

constexpr int THREADS = adjoint::THREADS;

// rows of M that touch a body, per body (CSR): entry = 2 row + half (half 1: the body is the child of the row's joint, columns 12..23)
struct Touch { const int* ptr; const int* ent; };

template <class TIO> struct Args {
    const TIO* DZ;          // [H][B][nx][nx]
    const TIO* DU;          // [H][B][nu][nx]
    const TIO* OBS;         // [H+1][B][nobs]
    const double* M;        // [H+1][B][nobs][24] compact observation Jacobians (M[H] is read only with G_obs)
    const TIO* G;           // [H][B][nx] (cot_space 0) or [H][B][13 Nb] (cot_space 1)
    const TIO* Z;           // [H][B][13 Nb], cot_space 1 only
    const TIO* G_u;         // [H][B][nu] or null
    const TIO* G_obs;       // [H+1][B][nobs] or null
    const int* status;      // [H][B] or null
    const TIO *W, *mean, *scale;    // [Bw][na][nobs], [nobs] or null, [nobs] or null
    Touch touch;
    TIO *gW, *gbias;        // per_env 1: [B][na][nobs], [B][na] (each may be null)
    double* acc_out;        // per_env 0: [B][na (nobs + 1)] fp64 workspace (gW rows, then gbias), or null
    TIO* gU;                // [H][B][nu] or null
    TIO* gz;                // [B][nx] or null
    int H, B, nx, nu, nobs, act_off, na, per_env, cot_space;
};

inline size_t lds_bytes(int nx, int nu, int nobs, int na) { return ((size_t)4 * nx + nu + 2 * (size_t)nobs + (size_t)na * (nobs + 1)) * sizeof(double); }

#if defined(__HIPCC__)
typedef coords::Dual<24> D24;
// a body state seeded with its 12 tangent directions [x, v, phi, omega] starting at direction d0: q (x) (1, phi)
__device__ __forceinline__ coords::PoseVel<D24> seed_body(const coords::PoseVel<double>& p, int d0) {
    using namespace coords;
    PoseVel<D24> s;
    for (int i = 0; i < 3; ++i) { s.x[i] = D24::seed(p.x[i], d0 + i); s.v[i] = D24::seed(p.v[i], d0 + 3 + i); s.w[i] = D24::seed(p.w[i], d0 + 9 + i); }
    D24 e[4] = {D24(1.0), D24::seed(0.0, d0 + 6), D24::seed(0.0, d0 + 7), D24::seed(0.0, d0 + 8)}, q0[4] = {D24(p.q[0]), D24(p.q[1]), D24(p.q[2]), D24(p.q[3])};
    qmulS(s.q, q0, e);
    return s;
}

// state 0 is read from z_first [B][13 Nb], the states 1 .. n-1 from z_rest [n-1][B][13 Nb] (a trajectory is (z0, Z); one array is (z, z + B 13 Nb))
constexpr int JAC_THREADS = 128;      // (a bound on the workgroup size: the Dual<24> evaluation wants more than the 128 registers a 1024-lane bound leaves)
template <class TIO>
__global__ void __launch_bounds__(JAC_THREADS) observation_jacobian_kernel(const NodeP<double>* nodes_, int Nb, int nu, double dt, int B, long long n, const TIO* z_first, const TIO* z_rest, double* M_) {
    using namespace coords;
    const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= n * B * Nb) return;
    const int k = (int)(tid % Nb); const long long sb = tid / Nb, st = sb / B; const int env = (int)(sb % B);
    const NodeP<double>* const nodes = DJ_GLOBAL_PTR(const NodeP<double>, nodes_);
    const NodeP<double>& P = nodes[k];
    const TIO* const ze = (st == 0 ? DJ_GLOBAL_PTR(const TIO, z_first) : DJ_GLOBAL_PTR(const TIO, z_rest) + (size_t)(st - 1) * B * 13 * Nb) + (size_t)env * 13 * Nb;
    const int nt = P.nu_t, nr = P.nu_r, nn = nt + nr;
    const bool has_parent = P.parent >= 0;
    const PoseVel<double> b0 = load_body<double>(ze, k), a0 = has_parent ? load_body<double>(ze, P.parent) : origin_body<double>();
    const PoseVel<D24> a = seed_body(a0, 0), b = seed_body(b0, 12);
    D24 ct[3], cr[3], vt[3], vr[3];
    joint_max2min(ct, cr, vt, vr, P, dt, a, b);
    double* const o = DJ_GLOBAL_PTR(double, M_) + ((size_t)sb * 2 * nu + 2 * P.u_off) * 24;
    for (int i = 0; i < 3; ++i) for (int d = 0; d < 24; ++d) {
        const bool live = d >= 12 || has_parent;                            // a joint on the origin has no parent columns: written as 0
        if (i < nt) { o[(size_t)i * 24 + d] = live ? ct[i].d[d] : 0.0; o[(size_t)(nn + i) * 24 + d] = live ? vt[i].d[d] : 0.0; }
        if (i < nr) { o[(size_t)(nt + i) * 24 + d] = live ? cr[i].d[d] : 0.0; o[(size_t)(nn + nt + i) * 24 + d] = live ? vr[i].d[d] : 0.0; }
    }
}

template <class TIO>
__global__ void __launch_bounds__(THREADS) rollout_policy_adjoint_kernel(const Args<TIO> A) {
    using namespace adjoint;
    typedef typename Piece<TIO>::type P;
    extern __shared__ __align__(16) double lds_[];      // lambda [2][nx] | g [2][nx] | gu [nu] | go [nobs] | ohat [nobs] | accumulators [na nobs + na]
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, team = tid / ROW, j = tid % ROW;
    const int H = A.H, B = A.B, nx = A.nx, nu = A.nu, nobs = A.nobs, na = A.na, act_off = A.act_off, nacc = na * nobs + na;
    const TIO* const G = DJ_GLOBAL_PTR(const TIO, A.G);   const TIO* const Z = DJ_GLOBAL_PTR(const TIO, A.Z);
    const TIO* const OBS = DJ_GLOBAL_PTR(const TIO, A.OBS); const double* const M = DJ_GLOBAL_PTR(const double, A.M);
    const TIO* const GU = DJ_GLOBAL_PTR(const TIO, A.G_u); const TIO* const GO = DJ_GLOBAL_PTR(const TIO, A.G_obs);
    const TIO* const W = DJ_GLOBAL_PTR(const TIO, A.W) + (A.per_env ? (size_t)b : (size_t)0) * na * nobs;
    const TIO* const mean = DJ_GLOBAL_PTR(const TIO, A.mean); const TIO* const scale = DJ_GLOBAL_PTR(const TIO, A.scale);
    const int* const status = DJ_GLOBAL_PTR(const int, A.status);
    const int* const tptr = DJ_GLOBAL_PTR(const int, A.touch.ptr); const int* const tent = DJ_GLOBAL_PTR(const int, A.touch.ent);
    TIO* const gU = DJ_GLOBAL_PTR(TIO, A.gU); TIO* const gz = DJ_GLOBAL_PTR(TIO, A.gz);
    const Columns<TIO> C = columns<TIO>(DJ_GLOBAL_PTR(const TIO, A.DZ), DJ_GLOBAL_PTR(const TIO, A.DU), B, nx, nu, nu);
    double* const lam_ = lds_; double* const g_ = lds_ + 2 * nx; double* const gu_ = lds_ + 4 * nx; double* const go_ = gu_ + nu;
    double* const oh_ = go_ + nobs; double* const acc_ = oh_ + nobs;
    // the cotangent of the state is the open-loop sweep's (adjoint::cotangent reads G, Z, B, nx, cot_space)
    const adjoint::Args<TIO> AG{nullptr, nullptr, A.G, A.Z, nullptr, nullptr, nullptr, H, B, nx, nu, A.cot_space};

    auto failed = [&](int k) { return status != nullptr && status[(size_t)k * B + b] != 0; };
    auto items_of = [&](int k) { return (k < 0 || failed(k)) ? 0 : items(C, 0); };
    // M_k^T go for column c: the rows that touch the column's body, in the order of the table
    auto pull = [&](int k, int c) {
        const int body = c / 12, col = c - 12 * body;
        const double* const Mk = M + ((size_t)k * B + b) * nobs * 24;
        double s = 0.0;
        for (int e = tptr[body]; e < tptr[body + 1]; ++e) { const int rh = tent[e], r = rh >> 1; s = fma(Mk[(size_t)r * 24 + (rh & 1) * 12 + col], go_[r], s); }
        return s;
    };
    auto put_ohat = [&](int k) {
        for (int i = tid; i < nobs; i += THREADS)
            oh_[i] = ((double)OBS[((size_t)k * B + b) * nobs + i] - (mean ? (double)mean[i] : 0.0)) * (scale ? (double)scale[i] : 1.0);
    };

    for (int e = tid; e < nacc; e += THREADS) acc_[e] = 0.0;
    for (int c = tid; c < nx; c += THREADS) g_[((H - 1) & 1) * nx + c] = cotangent(AG, G, Z, H - 1, b, c);
    put_ohat(H - 1);
    if (GO) {                                                               // lambda <- M_H^T GO_H  (+ g_{H-1}, where it is read)
        for (int i = tid; i < nobs; i += THREADS) go_[i] = (double)GO[((size_t)H * B + b) * nobs + i];
        __syncthreads();
        for (int c = tid; c < nx; c += THREADS) lam_[c] = pull(H, c);
    } else
        for (int c = tid; c < nx; c += THREADS) lam_[c] = 0.0;
    int p = 0, nit = items_of(H - 1);
    P buf0[COLS], buf1[COLS];
    if (nit) issue(C, H - 1, b, 0, 0, team, j, buf0);
    __syncthreads();
    for (int k = H - 1; k >= 0; --k) {
        const double* lam = lam_ + p * nx; const double* gk = g_ + (k & 1) * nx; double* lam_next = lam_ + (p ^ 1) * nx;
        const int nit_next = items_of(k - 1);
        const size_t kb = (size_t)k * B + b;
        if (k > 0) for (int c = tid; c < nx; c += THREADS) g_[((k - 1) & 1) * nx + c] = cotangent(AG, G, Z, k - 1, b, c);
        double acc[COLS];
#pragma unroll
        for (int i = 0; i < COLS; ++i) acc[i] = 0.0;
        auto put = [&](int c, double mine) { if (c >= nx) gu_[c - nx] = mine; else lam_next[c] = mine; };
        auto stage = [&](int it, const P (&cur)[COLS], P (&nxt)[COLS]) {
            const bool more = it + 1 < nit;
            issue(C, (more || !nit_next) ? k : k - 1, b, 0, more ? it + 1 : nit_next ? 0 : it, team, j, nxt);
            consume(C, 0, it, team, j, lam, gk, cur, acc, put);
        };
        for (int it = 0; it < nit; it += 2) { stage(it, buf0, buf1); stage(it + 1, buf1, buf0); }
        if (failed(k)) {                                                    // nothing flows through a failed step: DZ^T lambda = 0, DU^T lambda = 0
            for (int c = tid; c < nx; c += THREADS) lam_next[c] = 0.0;
            for (int c = tid; c < nu; c += THREADS) gu_[c] = 0.0;
            if (nit_next) issue(C, k - 1, b, 0, 0, team, j, buf0);
        }
        __syncthreads();
        // ---- phase (i): gu -> gU, go, the accumulators.  a_i = gu[act_off + i] + GU[act_off + i], formed by every lane that needs it (the same bits) ----
        auto act = [&](int i) { return gu_[act_off + i] + (GU ? (double)GU[kb * nu + act_off + i] : 0.0); };
        if (gU) for (int c = tid; c < nu; c += THREADS) gU[kb * nu + c] = (TIO)(gu_[c] + (GU ? (double)GU[kb * nu + c] : 0.0));
        for (int i = tid; i < nobs; i += THREADS) {
            double s = 0.0;
            for (int r = 0; r < na; ++r) s = fma((double)W[(size_t)r * nobs + i], act(r), s);
            go_[i] = (scale ? (double)scale[i] : 1.0) * s + (GO ? (double)GO[kb * nobs + i] : 0.0);
        }
        for (int e = tid; e < nacc; e += THREADS) {
            if (e < na * nobs) { const int r = e / nobs, i = e - r * nobs; acc_[e] = fma(act(r), oh_[i], acc_[e]); }
            else acc_[e] += act(e - na * nobs);
        }
        __syncthreads();
        // ---- phase (ii): lam_next += M_k^T go; the observation of the next step to come goes to LDS (its last reader was phase (i)) ----
        for (int c = tid; c < nx; c += THREADS) {
            const double v = lam_next[c] + pull(k, c);
            if (k > 0) lam_next[c] = v;
            else if (gz) gz[(size_t)b * nx + c] = (TIO)v;
        }
        if (k > 0) put_ohat(k - 1);
        __syncthreads();
        p ^= 1; nit = nit_next;
    }
    // the accumulators: rounded once (one policy per environment), or handed to the reduction as fp64 (shared policy)
    if (A.acc_out) {
        double* const out = DJ_GLOBAL_PTR(double, A.acc_out) + (size_t)b * nacc;
        for (int e = tid; e < nacc; e += THREADS) out[e] = acc_[e];
    } else {
        TIO* const gW = DJ_GLOBAL_PTR(TIO, A.gW); TIO* const gb = DJ_GLOBAL_PTR(TIO, A.gbias);
        if (gW) for (int e = tid; e < na * nobs; e += THREADS) gW[(size_t)b * na * nobs + e] = (TIO)acc_[e];
        if (gb) for (int e = tid; e < na; e += THREADS) gb[(size_t)b * na + e] = (TIO)acc_[na * nobs + e];
    }
}

// shared policy: out[e] = sum_b acc[b][e]; the entries [0, nW) go to gW, [nW, nacc) to gbias (each may be null)
template <class TIO>
__global__ void __launch_bounds__(THREADS) policy_reduce_kernel(const double* acc_, int B, int nacc, int nW, TIO* gW_, TIO* gbias_) {
    using namespace adjoint;
    const int tid = (int)threadIdx.x, j = tid % ROW, e = (int)blockIdx.x * (THREADS / ROW) + tid / ROW;
    const bool have = e < nacc;                                             // (no early return: row_sum sees all sixteen lanes of the row)
    const double* const acc = DJ_GLOBAL_PTR(const double, acc_);
    double s = 0.0;
    for (int b = j; b < B; b += ROW) s += have ? acc[(size_t)b * nacc + e] : 0.0;
    s = row_sum(s);
    if (have && j == 0) {
        TIO* const gW = DJ_GLOBAL_PTR(TIO, gW_); TIO* const gb = DJ_GLOBAL_PTR(TIO, gbias_);
        if (e < nW) { if (gW) gW[e] = (TIO)s; } else if (gb) gb[e - nW] = (TIO)s;
    }
}
#endif

}  // namespace padjoint
}  // namespace dj
