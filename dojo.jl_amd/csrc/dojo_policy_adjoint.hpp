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
//   rollout_policy_adjoint_kernel  one workgroup of 256 lanes per environment, one launch for all H steps.  DZ and DU go through the step loop of
//       dojo_adjoint.hpp (adjoint::sweep: 16-byte loads, two register buffers that take turns, row_sum, the next item in flight across the barriers);
//       gu lands in LDS as fp64.  Two short phases follow per step (the loop's `after` hook), each behind a barrier:
//         (i)  lanes c < nu round gu to gU; lanes j < nobs form go_j = scale_j sum_i W[i][j] a_i + GO_j (i ascending, W read coalesced along nobs); the
//              na nobs + na accumulators of gW / gbias live in LDS as fp64, entry e owned by lane e mod 256 (no races); ohat_k is in LDS, formed from the
//              recorded OBS[k] one phase earlier.
//         (ii) lanes over the columns c < nx add sum_r M[r][.] go_r to lam_next[c], r over the rows that touch body c / 12 -- its own joint's rows (child
//              half) and those of every joint whose parent it is -- in the ascending order of a CSR table (row, half) per body that the host builds once;
//              ohat_{k-1} goes to LDS.
//       LDS: lambda and g double-buffered (4 nx), gu (nu), go and ohat (2 nobs), the accumulators (na (nobs + 1)) doubles: Ant 7 KB, Atlas 30 KB.
//       All arithmetic is fp64, outputs are rounded once, no atomics: the summation order is fixed by (nx, nu, na, nobs, topology, dtype) alone.
//       Everything but the middle of phase (i) -- W and the accumulators -- is shared with the network's sweep (dojo_mlp.hpp): the argument record
//       Common and the per-workgroup Closed below.
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

// what the two closed-loop sweeps (this one, and the network's in dojo_mlp.hpp) are given alike: the record, the cotangents, the outputs that do not
// depend on the kind of policy, the sizes
template <class TIO> struct Common {
    const TIO* DZ;          // [H][B][nx][nx]
    const TIO* DU;          // [H][B][nu][nx]
    const TIO* OBS;         // [H+1][B][nobs]
    const double* M;        // [H+1][B][nobs][24] compact observation Jacobians (M[H] is read only with G_obs)
    const TIO* G;           // [H][B][nx] (cot_space 0) or [H][B][13 Nb] (cot_space 1)
    const TIO* Z;           // [H][B][13 Nb], cot_space 1 only
    const TIO* G_u;         // [H][B][nu] or null
    const TIO* G_obs;       // [H+1][B][nobs] or null
    const int* status;      // [H][B] or null
    const TIO *mean, *scale;    // [nobs] or null, [nobs] or null
    Touch touch;
    TIO* gU;                // [H][B][nu] or null
    TIO* gz;                // [B][nx] or null
    int H, B, nx, nu, nobs, act_off, per_env, cot_space;
};
template <class TIO> struct Args {
    Common<TIO> c;
    const TIO* W;           // [Bw][na][nobs]
    TIO *gW, *gbias;        // per_env 1: [B][na][nobs], [B][na] (each may be null)
    double* acc_out;        // per_env 0: [B][na (nobs + 1)] fp64 workspace (gW rows, then gbias), or null
    int na;
};

inline size_t lds_bytes(int nx, int nu, int nobs, int na) { return ((size_t)4 * nx + nu + 2 * (size_t)nobs + (size_t)na * (nobs + 1)) * sizeof(double); }

#if defined(__HIPCC__)
typedef coords::Dual<24> D24;

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
    const PoseVel<D24> a = seed_body<24>(a0, 0), b = seed_body<24>(b0, 12);
    D24 ct[3], cr[3], vt[3], vr[3];
    joint_max2min(ct, cr, vt, vr, P, dt, a, b);
    double* const o = DJ_GLOBAL_PTR(double, M_) + ((size_t)sb * 2 * nu + 2 * P.u_off) * 24;
    for (int i = 0; i < 3; ++i) for (int d = 0; d < 24; ++d) {
        const bool live = d >= 12 || has_parent;                            // a joint on the origin has no parent columns: written as 0
        if (i < nt) { o[(size_t)i * 24 + d] = live ? ct[i].d[d] : 0.0; o[(size_t)(nn + i) * 24 + d] = live ? vt[i].d[d] : 0.0; }
        if (i < nr) { o[(size_t)(nt + i) * 24 + d] = live ? cr[i].d[d] : 0.0; o[(size_t)(nn + nt + i) * 24 + d] = live ? vr[i].d[d] : 0.0; }
    }
}

// ---- what the two closed-loop sweeps do alike around adjoint::sweep, per workgroup (environment b) ----
// LDS behind lambda and g: gu [nu] | go [nobs] | ohat [nobs], then the kernel's own (rest()).  A step of either sweep is
//     the columns (put / failed_step): lam_next <- DZ_k^T lambda, gu <- DU_k^T lambda, or zeros
//     phase (i), the kernel's own:     round_gU(k); a = act(k, .); the accumulators; set_go(k, j, sum_i W[i][j] a_i or delta_0[j])
//     phase (ii):                      lam_next += M_k^T go (k = 0: -> gz); ohat_{k-1} to LDS
// each behind a barrier.
template <class TIO> struct Closed {
    const TIO *OBS, *GU, *GO, *mean, *scale;
    const double* M;
    const int *tptr, *tent;
    TIO *gU, *gz;
    double *gu_, *go_, *oh_;
    int b, tid, B, nx, nu, nobs, act_off;

    __device__ __forceinline__ Closed(const Common<TIO>& A, double* lds)
        : OBS(DJ_GLOBAL_PTR(const TIO, A.OBS)), GU(DJ_GLOBAL_PTR(const TIO, A.G_u)), GO(DJ_GLOBAL_PTR(const TIO, A.G_obs)), mean(DJ_GLOBAL_PTR(const TIO, A.mean)),
          scale(DJ_GLOBAL_PTR(const TIO, A.scale)), M(DJ_GLOBAL_PTR(const double, A.M)), tptr(DJ_GLOBAL_PTR(const int, A.touch.ptr)), tent(DJ_GLOBAL_PTR(const int, A.touch.ent)),
          gU(DJ_GLOBAL_PTR(TIO, A.gU)), gz(DJ_GLOBAL_PTR(TIO, A.gz)), gu_(lds + 4 * A.nx), go_(gu_ + A.nu), oh_(go_ + A.nobs),
          b((int)blockIdx.x), tid((int)threadIdx.x), B(A.B), nx(A.nx), nu(A.nu), nobs(A.nobs), act_off(A.act_off) {}
    __device__ __forceinline__ double* rest() const { return oh_ + nobs; }
    __device__ __forceinline__ adjoint::Columns<TIO> columns(const Common<TIO>& A) const {
        return adjoint::columns<TIO>(DJ_GLOBAL_PTR(const TIO, A.DZ), DJ_GLOBAL_PTR(const TIO, A.DU), B, nx, nu, nu);
    }
    // M_k^T go for column c: the rows that touch the column's body, in the order of the table
    __device__ __forceinline__ double pull(int k, int c) const {
        const int body = c / 12, col = c - 12 * body;
        const double* const Mk = M + ((size_t)k * B + b) * nobs * 24;
        double s = 0.0;
        for (int e = tptr[body]; e < tptr[body + 1]; ++e) { const int rh = tent[e], r = rh >> 1; s = fma(Mk[(size_t)r * 24 + (rh & 1) * 12 + col], go_[r], s); }
        return s;
    }
    // ohat_k from the recorded, rounded OBS[k]
    __device__ __forceinline__ void put_ohat(int k) const {
        for (int i = tid; i < nobs; i += THREADS)
            oh_[i] = ((double)OBS[((size_t)k * B + b) * nobs + i] - (mean ? (double)mean[i] : 0.0)) * (scale ? (double)scale[i] : 1.0);
    }
    // lam_[0 .. nx) <- M_H^T GO_H  (+ g_{H-1}, where it is read); contains a barrier with G_obs, which is uniform over the launch
    __device__ __forceinline__ void first_lambda(int H, double* lam_) const {
        if (GO) {
            for (int i = tid; i < nobs; i += THREADS) go_[i] = (double)GO[((size_t)H * B + b) * nobs + i];
            __syncthreads();
            for (int c = tid; c < nx; c += THREADS) lam_[c] = pull(H, c);
        } else
            for (int c = tid; c < nx; c += THREADS) lam_[c] = 0.0;
    }
    __device__ __forceinline__ void put(int c, double mine, double* lam_next) const { if (c >= nx) gu_[c - nx] = mine; else lam_next[c] = mine; }
    __device__ __forceinline__ void failed_step(double* lam_next) const {       // nothing flows through a failed step: DZ^T lambda = 0, DU^T lambda = 0
        for (int c = tid; c < nx; c += THREADS) lam_next[c] = 0.0;
        for (int c = tid; c < nu; c += THREADS) gu_[c] = 0.0;
    }
    // a_i = gu[act_off + i] + GU[act_off + i], formed by every lane that needs it (the same bits)
    __device__ __forceinline__ double act(int k, int i) const { return gu_[act_off + i] + (GU ? (double)GU[((size_t)k * B + b) * nu + act_off + i] : 0.0); }
    __device__ __forceinline__ void round_gU(int k) const {
        const size_t kb = (size_t)k * B + b;
        if (gU) for (int c = tid; c < nu; c += THREADS) gU[kb * nu + c] = (TIO)(gu_[c] + (GU ? (double)GU[kb * nu + c] : 0.0));
    }
    __device__ __forceinline__ void set_go(int k, int i, double s) const {
        go_[i] = (scale ? (double)scale[i] : 1.0) * s + (GO ? (double)GO[((size_t)k * B + b) * nobs + i] : 0.0);
    }
    // phase (ii): lam_next += M_k^T go; the observation of the next step to come goes to LDS (its last reader was phase (i)).  The caller's barrier follows.
    __device__ __forceinline__ void phase_ii(int k, double* lam_next) const {
        for (int c = tid; c < nx; c += THREADS) {
            const double v = lam_next[c] + pull(k, c);
            if (k > 0) lam_next[c] = v;
            else if (gz) gz[(size_t)b * nx + c] = (TIO)v;
        }
        if (k > 0) put_ohat(k - 1);
    }
};

template <class TIO>
__global__ void __launch_bounds__(THREADS) rollout_policy_adjoint_kernel(const Args<TIO> A) {
    extern __shared__ __align__(16) double lds_[];      // lambda [2][nx] | g [2][nx] | gu [nu] | go [nobs] | ohat [nobs] | accumulators [na nobs + na]
    const Closed<TIO> S(A.c, lds_);
    const int b = S.b, tid = S.tid, nx = S.nx, nobs = S.nobs, na = A.na, nacc = na * nobs + na;
    const TIO* const W = DJ_GLOBAL_PTR(const TIO, A.W) + (A.c.per_env ? (size_t)b : (size_t)0) * na * nobs;
    double* const acc_ = S.rest();

    for (int e = tid; e < nacc; e += THREADS) acc_[e] = 0.0;
    S.put_ohat(A.c.H - 1);
    S.first_lambda(A.c.H, lds_);
    adjoint::sweep(S.columns(A.c), adjoint::cot_of<TIO>(A.c), DJ_GLOBAL_PTR(const int, A.c.status), A.c.H, b, lds_, lds_ + 2 * nx,
        [](int) { return 0; },
        [&](int, int c, double mine, double* lam_next) { S.put(c, mine, lam_next); },
        [&](int, double* lam_next) { S.failed_step(lam_next); },
        [&](int k, double* lam_next) {
            // ---- phase (i): gu -> gU, go, the accumulators ----
            S.round_gU(k);
            for (int i = tid; i < nobs; i += THREADS) {
                double s = 0.0;
                for (int r = 0; r < na; ++r) s = fma((double)W[(size_t)r * nobs + i], S.act(k, r), s);
                S.set_go(k, i, s);
            }
            for (int e = tid; e < nacc; e += THREADS) {
                if (e < na * nobs) { const int r = e / nobs, i = e - r * nobs; acc_[e] = fma(S.act(k, r), S.oh_[i], acc_[e]); }
                else acc_[e] += S.act(k, e - na * nobs);
            }
            __syncthreads();
            S.phase_ii(k, lam_next);
            __syncthreads();
        });
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
