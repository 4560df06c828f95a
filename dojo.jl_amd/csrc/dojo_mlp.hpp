// dojo_mlp.hpp -- closed-loop rollouts whose controller is a small tanh network (dojo_rollout_mlp_dev) and reverse mode through them
// (dojo_rollout_mlp_adjoint_dev).  The affine policy of dojo_policy.hpp / dojo_policy_adjoint.hpp is the one-layer case, and both kernels here are
// those kernels with the mat-vec replaced by a stack of them: the operation order of every sum is kept, so that n_layers = 1 gives their bits.
//
// Per environment b and step k, L = n_layers, widths n_0 = nobs, n_1 .. n_{L-1} hidden, n_L = na:
//
//     o_k  = the observation of dojo_policy.hpp, rounded once to the ABI type, -> OBS[k][b]
//     h_0  = (o_k - mean) .* scale                                     from the ROUNDED o_k, fp64
//     p_l  = b_l + W_l h_{l-1},   h_l = tanh(p_l)    l = 1 .. L-1      fp64;  h_1 .. h_{L-1} -> ACT[k][b] (fp64 whatever the ABI type)
//     a    = b_L + W_L h_{L-1}                                         (no activation on the output layer)
//     u    = U_ff[k][b];  u[act_off + i] += a_i                        rounded once, -> U_out[k][b], read by step k
//
// theta is one flat vector per policy, layer after layer: W_l row-major [n_l][n_{l-1}], then b_l [n_l]; P = sum_l n_l (n_{l-1} + 1) entries.
//
// rollout_mlp_kernel  one wavefront per environment, four per 256-lane workgroup (the mapping of rollout_policy_kernel).
//   Phase A  the observation: policy::observe, the function rollout_policy_kernel calls; h_0 to LDS.
//   Layers   per output i of a layer: lane j accumulates W_l[i][j] h_{l-1}[j], W_l[i][j + 64] h_{l-1}[j + 64], ... with fma in ascending order, the 64
//            partial sums meet in policy::wave_sum, b_l[i] is added in front.  Lane i mod 64 keeps p_l[i]; after 64 outputs (or the layer's last) every
//            lane takes the tanh of its own at once -- one tanh per 64 outputs, not one per output -- and h_l goes to LDS and to ACT.  A barrier
//            separates the layers.  The output layer is phase B of rollout_policy_kernel.
//   LDS: [4][nobs + nh] doubles, nh = n_1 + .. + n_{L-1}.  No atomics; the summation order is fixed by the widths alone.
//
// rollout_mlp_adjoint_kernel  one workgroup of 256 lanes per environment, one launch for all H steps: rollout_policy_adjoint_kernel (its argument
//   record padjoint::Common, its per-workgroup padjoint::Closed, the step loop adjoint::sweep) with the middle of phase (i)
//   replaced by back-propagation through the layers, h_l read from the recorded ACT[k][b] (no tanh, no forward pass):
//
//     delta_L = gu[act_off .. act_off + na - 1]          (gu = DU_k^T lambda + GU_k -> gU[k])
//     for l = L .. 1:   g b_l += delta_l;   g W_l += delta_l h_{l-1}^T;   delta_{l-1} = (W_l^T delta_l) .* (1 - h_{l-1}^2)    (no factor for l = 1)
//     go = scale .* delta_0 + GO_k;   lambda = DZ_k^T lambda + M_k^T go (+ g_{k-1})
//
//   W_l^T delta_l is summed with i ascending by the lanes j < n_{l-1} (W_l read coalesced along n_{l-1}); 1 - h^2 is fma(-h, h, 1).
//   THE ACCUMULATORS live in an fp64 workspace in global memory, [B][P], row b owned by workgroup b and entry e of a layer's block by lane e mod 256
//   for the whole launch: one fma per entry and step, the first step writes (no read, no zero fill), the last one writes the result -- rounded once
//   to gtheta (one policy per environment) or as fp64 for policy_reduce_kernel (shared policy).  LDS would hold 64 KB / 8 = 8192 entries less the
//   sweep's own, which a [28, 300, 8] policy (11108) exceeds; registers would need a compile-time cap per lane and a second path behind it.  The
//   workspace has no limit of its own, is read and written coalesced, and costs 16 P bytes of traffic per environment and step.
//   LDS: 4 nx + nu + 2 nobs + 2 wmax + nh doubles (wmax = the largest width: delta_l and delta_{l-1}; nh: the activations of the step).
#pragma once
#include <hip/hip_runtime.h>
#include "dojo_math.hpp"
#include "dojo_coords.hpp"
#include "dojo_adjoint.hpp"
#include "dojo_policy.hpp"
#include "dojo_policy_adjoint.hpp"

namespace dj {
namespace mlp {

constexpr int MAX_LAYERS = 4;

// what the widths determine, computed once on the host
struct Shape {
    int L;                          // layers
    int width[MAX_LAYERS + 1];      // n_0 .. n_L
    int toff[MAX_LAYERS];           // toff[l - 1]: where W_l starts in theta (b_l follows its n_l n_{l-1} entries)
    int hoff[MAX_LAYERS];           // hoff[l]: where h_l starts in a row of ACT, l = 1 .. L-1 (hoff[0] unused)
    int nh, wmax;                   // n_1 + .. + n_{L-1}; the largest width
    long long P;                    // entries of theta
};
// widths n[0 .. L], each >= 1, 1 <= L <= MAX_LAYERS (checked by the caller).  The sums are formed in 64 bits and saturate just above INT_MAX (a layer alone
// can reach 2^62): a P that exceeds an int is what the caller refuses, and the offsets of such a shape are never used.
inline Shape shape(int L, const int* n) {
    constexpr long long LIM = 0x7fffffffLL;
    Shape s{};
    s.L = L;
    long long P = 0, nh = 0; int wmax = 0;
    for (int l = 0; l <= L; ++l) { s.width[l] = n[l]; if (n[l] > wmax) wmax = n[l]; }
    for (int l = 1; l <= L; ++l) {
        s.toff[l - 1] = (int)(P < LIM ? P : LIM);
        const long long add = (long long)n[l] * ((long long)n[l - 1] + 1);
        P = (P > LIM || add > LIM) ? LIM + 1 : P + add;
        if (l < L) { s.hoff[l] = (int)(nh < LIM ? nh : LIM); nh += n[l]; }
    }
    s.nh = (int)(nh < LIM ? nh : LIM); s.wmax = wmax; s.P = P;
    return s;
}
inline size_t lds_bytes(int nobs, int nh) { return (size_t)policy::ENVS * ((size_t)nobs + (size_t)nh) * sizeof(double); }
inline size_t adjoint_lds_bytes(int nx, int nu, int nobs, int wmax, int nh) {
    return ((size_t)4 * nx + nu + 2 * (size_t)nobs + 2 * (size_t)wmax + (size_t)nh) * sizeof(double);
}

template <class TIO> struct Args {
    const NodeP<double>* nodes;
    const TIO* z;                       // [B][13 Nb]: the state the step starts from
    const TIO* csg;                     // [B][8 Nc]: [s; gamma] per contact of the previous step; null = the neutral 1.0
    const TIO *theta, *mean, *scale;    // [Bw][P], [nobs] or null, [nobs] or null
    const TIO* uff;                     // [B][nu] of this step or null
    TIO* obs;                           // [B][nobs] of this step or null
    TIO* u;                             // [B][nu] of this step; null = observation only
    double* act;                        // [B][nh] of this step or null
    int env0, nenv;                     // the environments of this launch (all pointers are batch-level)
    int Nb, nu, Nc, nobs, act_off, per_env, P;
    double dt;
    Shape s;
};

template <class TIO> struct AdjointArgs {
    padjoint::Common<TIO> c;
    const double* ACT;      // [H][B][nh] (null with L = 1)
    const TIO* theta;       // [Bw][P]
    double* ws;             // [B][P] fp64: the accumulators between the steps; with `shared` the result as well
    TIO* gtheta;            // [B][P], one policy per environment (may be null); unused with `shared`
    int shared, P;
    Shape s;
};

#if defined(__HIPCC__)
// the activation of the hidden layers: the device library's fp64 tanh
__device__ __forceinline__ double activation(double p) { return ::tanh(p); }

template <class TIO>
__global__ void __launch_bounds__(policy::THREADS) rollout_mlp_kernel(const Args<TIO> A) {
    constexpr int WAVE = policy::WAVE, ENVS = policy::ENVS;
    extern __shared__ __align__(16) double lds_[];                          // per wavefront: h_0 [nobs] | h_1 .. h_{L-1} [nh] (a row of ACT)
    const int tid = (int)threadIdx.x, wave = tid / WAVE, lane = tid % WAVE;
    const int e = (int)blockIdx.x * ENVS + wave;
    const bool live = e < A.nenv;
    const size_t env = (size_t)A.env0 + (live ? e : 0);
    const int nu = A.nu, nobs = A.nobs, L = A.s.L, nh = A.s.nh;
    const NodeP<double>* const nodes = DJ_GLOBAL_PTR(const NodeP<double>, A.nodes);
    const TIO* const ze = DJ_GLOBAL_PTR(const TIO, A.z) + env * 13 * A.Nb;
    const TIO* const csg = DJ_GLOBAL_PTR(const TIO, A.csg);
    const TIO* const mean = DJ_GLOBAL_PTR(const TIO, A.mean); const TIO* const scale = DJ_GLOBAL_PTR(const TIO, A.scale);
    TIO* const obs = A.obs ? DJ_GLOBAL_PTR(TIO, A.obs) + env * nobs : nullptr;
    double* const hs = lds_ + (size_t)wave * (nobs + nh);
    if (live) policy::observe<TIO>(A, nodes, ze, csg, mean, scale, env, lane, obs, hs);
    if (!A.u) return;                                                       // (uniform over the launch)
    __syncthreads();
    // (a wavefront whose environment does not exist does no work below, but reaches every barrier; `live` is uniform over the wavefront, so the DPP
    // sums see all 64 lanes)
    const TIO* const theta = DJ_GLOBAL_PTR(const TIO, A.theta) + (A.per_env ? env : (size_t)0) * (size_t)A.P;
    const TIO* const uff = A.uff ? DJ_GLOBAL_PTR(const TIO, A.uff) + env * nu : nullptr;
    TIO* const u = DJ_GLOBAL_PTR(TIO, A.u) + env * nu;
    double* const act = A.act ? DJ_GLOBAL_PTR(double, A.act) + env * nh : nullptr;
    const int na = A.s.width[L];
    if (live)
        for (int c = lane; c < nu; c += WAVE)
            if (c < A.act_off || c >= A.act_off + na) u[c] = uff ? uff[c] : (TIO)0.0;
    for (int l = 1; l <= L; ++l) {
        const int nin = A.s.width[l - 1], nout = A.s.width[l];
        if (live) {
            const TIO* const W = theta + A.s.toff[l - 1];
            const TIO* const bl = W + (size_t)nout * nin;
            const double* const hin = l == 1 ? hs : hs + nobs + A.s.hoff[l - 1];
            if (l < L) {
                double* const hout = hs + nobs + A.s.hoff[l];
                for (int i0 = 0; i0 < nout; i0 += WAVE) {
                    const int n = nout - i0 < WAVE ? nout - i0 : WAVE;
                    double mine = 0.0;
                    for (int ii = 0; ii < n; ++ii) {
                        const TIO* const Wi = W + (size_t)(i0 + ii) * nin;
                        double acc = 0.0;
                        for (int j = lane; j < nin; j += WAVE) acc = fma((double)Wi[j], hin[j], acc);
                        const double p = (double)bl[i0 + ii] + policy::wave_sum(acc);
                        if (lane == ii) mine = p;
                    }
                    if (lane < n) {
                        const double h = activation(mine);
                        hout[i0 + lane] = h;
                        if (act) act[A.s.hoff[l] + i0 + lane] = h;
                    }
                }
            } else {
                for (int i = 0; i < nout; ++i) {
                    const TIO* const Wi = W + (size_t)i * nin;
                    double acc = 0.0;
                    for (int j = lane; j < nin; j += WAVE) acc = fma((double)Wi[j], hin[j], acc);
                    const double a = (double)bl[i] + policy::wave_sum(acc);
                    const int c = A.act_off + i;
                    if (lane == c % WAVE) u[c] = (TIO)((uff ? (double)uff[c] : 0.0) + a);
                }
            }
        }
        if (l < L) __syncthreads();
    }
}

template <class TIO>
__global__ void __launch_bounds__(padjoint::THREADS) rollout_mlp_adjoint_kernel(const AdjointArgs<TIO> A) {
    constexpr int THREADS = padjoint::THREADS;
    extern __shared__ __align__(16) double lds_[];      // lambda [2][nx] | g [2][nx] | gu [nu] | go [nobs] | h_0 [nobs] | delta [2][wmax] | h_1 .. h_{L-1} [nh]
    const padjoint::Closed<TIO> S(A.c, lds_);
    const int b = S.b, tid = S.tid, H = A.c.H, B = S.B, nx = S.nx, L = A.s.L, nh = A.s.nh, wmax = A.s.wmax, na = A.s.width[L];
    const double* const ACT = DJ_GLOBAL_PTR(const double, A.ACT);
    const TIO* const theta = DJ_GLOBAL_PTR(const TIO, A.theta) + (A.c.per_env ? (size_t)b : (size_t)0) * (size_t)A.P;
    double* const ws = DJ_GLOBAL_PTR(double, A.ws) + (size_t)b * (size_t)A.P;
    TIO* const gth = (!A.shared && A.gtheta) ? DJ_GLOBAL_PTR(TIO, A.gtheta) + (size_t)b * (size_t)A.P : nullptr;
    double* const dl_ = S.rest(); double* const hk_ = dl_ + 2 * wmax;
    // h_1 .. h_{L-1} of step k from the recorded ACT[k] (h_0 is the affine sweep's ohat)
    auto put_act = [&](int k) { for (int i = tid; i < nh; i += THREADS) hk_[i] = ACT[((size_t)k * B + b) * nh + i]; };

    S.put_ohat(H - 1); put_act(H - 1);
    S.first_lambda(H, lds_);
    adjoint::sweep(S.columns(A.c), adjoint::cot_of<TIO>(A.c), DJ_GLOBAL_PTR(const int, A.c.status), H, b, lds_, lds_ + 2 * nx,
        [](int) { return 0; },
        [&](int, int c, double mine, double* lam_next) { S.put(c, mine, lam_next); },
        [&](int, double* lam_next) { S.failed_step(lam_next); },
        [&](int k, double* lam_next) {
            // ---- phase (i): gu -> gU; delta_L = gu[act_off ..] + GU[act_off ..] to LDS ----
            S.round_gU(k);
            int cur = 0;
            for (int i = tid; i < na; i += THREADS) dl_[i] = S.act(k, i);
            __syncthreads();
            // ---- back-propagation, l = L .. 1: the accumulators of layer l, then delta_{l-1} (l = 1: go) ----
            const bool first = k == H - 1, last = k == 0;
            for (int l = L; l >= 1; --l) {
                const int nin = A.s.width[l - 1], nout = A.s.width[l], t0 = A.s.toff[l - 1], nW = nout * nin;
                const double* const dl = dl_ + cur * wmax; double* const dprev = dl_ + (cur ^ 1) * wmax;
                const double* const hin = l == 1 ? S.oh_ : hk_ + A.s.hoff[l - 1];
                // entry e = r nin + c of W_l: (r, c) advance by 256 without a division inside the loop
                {
                    const int qs = THREADS / nin, rs = THREADS - qs * nin;
                    int r = tid / nin, c = tid - r * nin;
                    for (int e = tid; e < nW; e += THREADS) {
                        const double v = fma(dl[r], hin[c], first ? 0.0 : ws[t0 + e]);
                        if (!last || A.shared) ws[t0 + e] = v; else if (gth) gth[t0 + e] = (TIO)v;
                        r += qs; c += rs; if (c >= nin) { c -= nin; ++r; }
                    }
                    for (int e = tid; e < nout; e += THREADS) {
                        const double v = (first ? 0.0 : ws[t0 + nW + e]) + dl[e];
                        if (!last || A.shared) ws[t0 + nW + e] = v; else if (gth) gth[t0 + nW + e] = (TIO)v;
                    }
                }
                const TIO* const W = theta + t0;
                for (int i = tid; i < nin; i += THREADS) {
                    double s = 0.0;
                    for (int r = 0; r < nout; ++r) s = fma((double)W[(size_t)r * nin + i], dl[r], s);
                    if (l > 1) dprev[i] = s * fma(-hin[i], hin[i], 1.0);
                    else S.set_go(k, i, s);
                }
                cur ^= 1;
                __syncthreads();
            }
            // ---- phase (ii); the activations of the next step to come go to LDS as well (their last reader was the loop above) ----
            S.phase_ii(k, lam_next);
            if (k > 0) put_act(k - 1);
            __syncthreads();
        });
}
#endif

}  // namespace mlp
}  // namespace dj
