// dojo_riccati.hpp -- the backward pass of iLQR (IterativeLQR's backward_pass!, as driven by the reference's examples/trajectory_optimization over
// get_minimal_gradients!) in minimal coordinates, all H steps of every environment in ONE launch (dojo_riccati_dev).
//
// Per environment b, with n = 2 nu, m = na, A_k = jx of step k [n x n], B_k = the columns act_off .. act_off + m - 1 of ju of step k [n x m]:
//
//     Vx <- lx_H;  Vxx <- lxx_H;  dV <- (0, 0);  fail <- 0
//     for k = H-1 .. 0:   failed step (status[k][b] != 0):  A_k, B_k are never loaded and count as zero
//         Qx  = lx_k + A^T Vx            Qu  = lu_k + B^T Vx
//         Qxx = lxx_k + A^T Vxx A        Qux = lux_k + B^T Vxx A        Quu = luu_k + B^T Vxx B
//         Qreg = Quu + mu[b] I = L L^T;  a pivot that is not > 0 or not finite:  fail <- k + 1, stop this environment
//         kff = -Qreg^-1 Qu              K = -Qreg^-1 Qux
//         dV[0] += kff^T Qu              dV[1] += 1/2 kff^T Quu kff
//         Vx  = Qx  + K^T Quu kff + K^T Qu  + Qux^T kff
//         Vxx = Qxx + K^T Quu K   + K^T Qux + Qux^T K;   Vxx <- (Vxx + Vxx^T) / 2
//
// What decides the mapping is the latency of one step (Ant: 0.1 Mflop, H steps strictly in sequence) and, for Atlas (n 72, m 30), the 64 KB of LDS: Vxx and
// [A B] alone are 41 KB + 59 KB in fp64.  One workgroup of 256 lanes per environment; N = n + m, F = [A B] (n x N), Q = [Qxx Qxu; Qux Quu] (N x N, symmetric).
//   * Vxx lives in LDS between the steps, SYMMETRIC-PACKED (lower triangle, n (n + 1) / 2 doubles: it is symmetrized at every step anyway), Vx next to it.
//   * Q = l + F^T (Vxx F) is accumulated in REGISTERS, output-stationary: the lower triangle of Q has N (N + 1) / 2 entries, entry e = tid + 256 q belongs to lane
//     tid for the whole launch (q < NQ, a template parameter: 3, 6, 12 or 24 accumulators per lane -- N <= 38, 54, 77, 110; Ant 36 -> 3, Quadruped 48 -> 6,
//     Atlas 102 -> 24).  Its (row, column) is decoded once.  The symmetric part of lxx_k, luu_k is what enters (the reference's final symmetrization does the same).
//   * T = [Vxx; Vx^T] F is formed R = 16 rows at a time (the extra row gives Qx, Qu): for a block of rows the lanes write F's rows (fp64) and T's rows into LDS
//     (T: one lane per column and group of 4 rows: a loaded F[i][j] feeds four sums; F comes from global memory, where consecutive lanes read consecutive
//     columns), barrier, every accumulator takes its R products F[k][r] T[k][c], barrier.  2 ceil((n + 1) / R) barriers: Ant 4, Atlas 10.  F of a step is read
//     ceil((n + 1) / R) + 1 times, from L2 after the first.
//   * Behind the last block Vxx is dead and so are the row buffers: K (m x n) takes Vxx's place, Qux, Quu and L the row buffers'.  The lanes that own them scatter
//     Qux and Quu (both triangles) to LDS; Qxx STAYS in its accumulators.
//   * Cholesky: wavefront 0 alone, lane i = row i, column by column (the pivot crosses the lanes with a shuffle, the columns already done are read from LDS behind a
//     wavefront-level fence: no workgroup barrier in the m columns).  m <= 64.
//   * The m-row solves are independent per right-hand side: one lane per column of [Qux | Qu] does its forward and backward substitution in place, in LDS, with no
//     synchronization at all.
//   * With Y = 1/2 Quu K + Qux (in place, over Qux) and g = 1/2 Quu kff + Qu:  K^T Quu K + K^T Qux + Qux^T K = K^T Y + Y^T K  (symmetric as written: the final
//     symmetrization is implicit) and K^T Quu kff + K^T Qu + Qux^T kff = K^T g + Y^T kff.  The owner of entry (r, c) of Qxx adds its m products and writes the new
//     packed Vxx.  8 more barriers per step.
//   * Everything is fp64; inputs are converted on load, outputs rounded once.  No atomics; every sum runs in an order fixed by (n, m): bit-identical from run to run,
//     independent of B and of the environment's place in the batch.
//   * Failure: the lanes leave together after writing zeros to K, kff of the steps <= k and to dV, Vx, Vxx.  Every element of every output is written in every case.
//
// LDS (dynamic), doubles:  n (n + 1) / 2  +  max(2 R N, m n + 2 m^2)  +  n + N + 3 m + 8   -- Ant (28, 8) 13 232 B, Quadruped (36, 12) 18 640 B,
// Atlas (72, 30) 54 880 B, Atlas with all 36 inputs 64 864 B.  Refused (DOJO_ERR_UNSUPPORTED, byte count in the text): more than 64 KB, N > 110, m > 64.
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage), NQ = 3 / 6 / 12 / 24: fp32 127 / 137 / 155 / 191 VGPRs, fp64 116 / 125 / 143 / 179; no AGPRs, no
// scratch, no VGPR spills in any of the eight instantiations (112 .. 138 SGPRs are parked in VGPR lanes, as in the other sweep kernels of this library: the thirteen
// array pointers of Args and the step's bases).  Ant runs four workgroups per CU, Atlas two (LDS).
//
// Not part of it: the forward pass as one fused call (it needs time-varying gains in the controller kernel: a follow-up), costs shared across the batch or given
// as diagonals, second-order dynamics terms (DDP), second-order constraint terms, kinematic loops.  Control limits and other constraints: the variants below.
//
// The control-limited variant (dojo_riccati_box_dev, include/dojo_hip_limits.h: the recursion, the solver and the failure codes are documented there) is this
// kernel over BoxArgs, every difference behind `if constexpr (BOX)`; the instantiations over Args keep the instructions they had before it existed.  Per step:
//   * in front of the Cholesky lane i of wavefront 0 forms lo'_i = lo_i - U_i and hi'_i (registers); !(lo' <= hi') anywhere: flag -1, code -(k + 1);
//   * K and kff are solved as above, unchanged -- kf is then the start point of the QP, and a step whose start point is not clipped is finished (its cost over
//     the unconstrained kernel: a ballot and one barrier);
//   * otherwise wavefront 0, lane = row, runs the projected Newton (box_qp): g = Qu + Qreg x per lane over column i of the symmetric Quu, the clamped set by
//     ballot, the masked Cholesky over L (box_factor: the column loop above with identity rows for clamped lanes), the direction by column-oriented substitutions
//     (box_solve: shuffles, the reciprocal pivots per lane), the trial step in LDS (dl) for the second mat-vec, the two scalar sums of a trial by a fixed
//     xor-butterfly (wave_add).  wave_sync() between dependent LDS accesses, no workgroup barrier inside.  Details fixed here: the pivots of the direction's
//     substitutions are multiplied by their reciprocals (the gains' solves divide, as above); f(x+) - f(x) is evaluated as g' dx + 1/2 dx' Qreg dx; a bad pivot
//     of a masked factor counts as a failed QP; qp_iters counts the factorizations inside the loop;
//   * a barrier; a failed QP leaves through the failure path (flag -1); a QP that ran: the lanes solve K again from Qux with the masked factor in L, clamped
//     rows written as zeros.
// LDS: the plan above + m doubles (dl): Ant 13 296 B, Quadruped 18 736 B, Atlas (72, 30) 55 120 B, Atlas with all 36 inputs 65 152 B (fits).  Resources, NQ = 3 / 6
// / 12 / 24: fp32 147 / 153 / 171 / 207 VGPRs, fp64 136 / 145 / 163 / 199; no AGPRs, no scratch, no VGPR spills (146 .. 178 SGPRs parked in VGPR lanes).  The Ant's
// fp32 build is over 128: three workgroups per CU where the unconstrained one runs four (4.06 ms against 3.11 ms with limits that clip nothing).
//
// The constrained variant (dojo_riccati_al_dev, include/dojo_hip_constraints.h: the recursion and the refusals are documented there) is the control-limited kernel
// over AlArgs (BOX holds for it too), every further difference behind `if constexpr (AL)`; the sixteen instantiations over Args and BoxArgs keep their instructions.
// The augmented-Lagrangian terms of nc constraint rows per stage, G' diag(w) G and G' y with G = [Cx Cu], never exist in memory (al_rows):
//   * behind the dynamics blocks of a step -- also of a failed one -- the rows go R = 16 at a time through the same row buffers, Fb = G, Tb = diag(w) G, and the same
//     accumulator loop; q += G' y is taken by lane j over the block's rows; two barriers per block;
//   * a row with w = y = 0 is not loaded, a block of 16 such rows is skipped with its barriers.  Lane l of every wavefront reads w, y of row l and a ballot gives
//     every wavefront the same mask: one load per 64 rows, issued a step ahead (w_next, y_next) so that its latency is hidden behind the step in between;
//   * the terminal stage: the owners of the packed Vxx entries load them into accumulators, run the same blocks over Cx_H alone and write them back;
//   * lim = NULL is lo = hi = NULL (U is then not read).  The host launches the control-limited kernel when nc = 0 and U is given: the same bits, fewer registers.
// LDS: box_lds_bytes, nothing on top (al_lds_bytes), whatever nc.  Resources, NQ = 3 / 6 / 12 / 24: see DESIGN.md 5k.
#pragma once
#include <hip/hip_runtime.h>
#include "dojo_math.hpp"
#include <type_traits>

namespace dj {
namespace riccati {

template <class TIO> struct Args {
    const TIO* A;           // [H][B][n][n]
    const TIO* Bm;          // [H][B][n][nu]
    const int* status;      // [H][B] or null
    const TIO *lx, *lu, *lxx, *luu, *lux, *mu;      // [H+1][B][n], [H][B][m], [H+1][B][n][n], [H][B][m][m], [H][B][m][n] or null, [B] or null
    TIO *K, *kff;           // [H][B][m][n], [H][B][m]
    int* fail;              // [B]
    TIO *dV, *Vx, *Vxx;     // [B][2], [B][n], [B][n][n]; each may be null
    int H, B, n, nu, m, act_off;
};

// the argument record of the control-limited variant (include/dojo_hip_limits.h): riccati_kernel<TIO, NQ, BoxArgs<TIO>>
template <class TIO> struct BoxArgs : Args<TIO> {
    const TIO *lo, *hi;     // [B][m]; either may be null
    const TIO* U;           // [H][B][nu]: the controls the limits are taken relative to
    long long* active;      // [H][B] or null: bit i = row i clamped
    int* iters;             // [H][B] or null
};

// the argument record of the constrained variant (include/dojo_hip_constraints.h): riccati_kernel<TIO, NQ, AlArgs<TIO>>.  lo, hi and U may all be null: no limits
template <class TIO> struct AlArgs : BoxArgs<TIO> {
    const TIO *Cx, *Cu, *w, *y;     // [H+1][B][nc][n] ([nc][n] when shared), [H][B][nc][m] ([nc][m] when shared) or null: zeros, [H+1][B][nc], [H+1][B][nc]
    int nc, shared;
};

constexpr int THREADS = 256, R = 16, RB = 4, MAX_M = 64;        // lanes per workgroup, rows of T per block, rows per lane in a block, rows of the one-wavefront Cholesky
inline int entries(int n, int m) { return (n + m) * (n + m + 1) / 2; }                                   // lower triangle of Q
inline int accumulators(int n, int m) {                                                                  // NQ of the instantiation that holds them, 0: none does
    const int e = entries(n, m);
    for (int nq : {3, 6, 12, 24}) if (e <= nq * THREADS) return nq;
    return 0;
}
inline size_t region1(int n, int m) { const size_t a = 2 * (size_t)R * (n + m), b = (size_t)m * n + 2 * (size_t)m * m; return a > b ? a : b; }
inline size_t lds_bytes(int n, int m) { return ((size_t)n * (n + 1) / 2 + region1(n, m) + (size_t)n + (n + m) + 3 * (size_t)m + 8) * sizeof(double); }
inline size_t box_lds_bytes(int n, int m) { return lds_bytes(n, m) + (size_t)m * sizeof(double); }      // + the trial step of the QP
inline size_t al_lds_bytes(int n, int m) { return box_lds_bytes(n, m); }                                // the constraint rows go through Fb, Tb: nothing on top, whatever nc

#if defined(__HIPCC__)
// LDS written by some lanes of a wavefront, read by others of the same wavefront: the hardware keeps a wavefront's LDS operations in order, the fence keeps the compiler from moving them
__device__ inline void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// ---- the box QP of a step (the BoxArgs variant): wavefront 0, lane i = row i; the lanes >= m carry zeros and an infinite box ----
__device__ __forceinline__ double wave_add(double v) {          // every lane gets the same bits: the sum of the 64 in the order of the butterfly
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}
// Qreg with the rows and columns of `set` replaced by the identity's = L L^T, as the Cholesky of the sweep; rinv: 1 / L[tid][tid].  false: a pivot is not > 0 or not finite
__device__ inline bool box_factor(const double* Quu, double* L, int m, double mu, unsigned long long set, int tid, double& rinv) {
    const bool mine = set >> tid & 1;
    for (int j = 0; j < m; ++j) {
        double s = 0.0;
        if (tid < m && tid >= j) {
            s = (mine || (set >> j & 1)) ? (tid == j ? 1.0 : 0.0) : Quu[tid * m + j] + (tid == j ? mu : 0.0);
#pragma unroll 2
            for (int p = 0; p < j; ++p) s = fma(-L[tid * m + p], L[j * m + p], s);
        }
        const double d = __shfl(s, j);
        if (!(d > 0.0) || !(d < __builtin_huge_val())) return false;
        const double rd = sqrt(d);
        if (tid < m && tid >= j) L[tid * m + j] = tid == j ? rd : s / rd;
        if (tid == j) rinv = 1.0 / rd;
        wave_sync();
    }
    return true;
}
// (L L^T)^-1 r, lane i holding r_i and the result's row i: column-oriented substitutions, the finished component crosses the lanes with a shuffle
__device__ inline double box_solve(const double* L, int m, int tid, double rinv, double s) {
    for (int p = 0; p < m; ++p) {
        const double y = __shfl(s * rinv, p);
        if (tid == p) s = y;
        if (tid > p && tid < m) s = fma(-L[tid * m + p], y, s);
    }
    for (int p = m - 1; p >= 0; --p) {
        const double x = __shfl(s * rinv, p);
        if (tid == p) s = x;
        if (tid < p) s = fma(-L[p * m + tid], x, s);
    }
    return s;
}
// kf: in, -Qreg^-1 Qu; out, argmin 1/2 x' Qreg x + qu' x over lo <= x <= hi by projected Newton (the header of include/dojo_hip_limits.h).  set: the clamped rows,
// it: the iterations.  -> 1: the clip changed nothing (L untouched), 2: solved, L holds box_factor(set), -1: failed
__device__ inline int box_qp(const double* Quu, double* L, double* kf, double* dl, const double* qu_, int m, double mu, double lo, double hi, int tid,
                             unsigned long long& set, int& it) {
    const bool valid = tid < m;
    const auto clip = [&](double v) { return v < lo ? lo : v > hi ? hi : v; };
    double x = valid ? kf[tid] : 0.0;
    set = 0; it = 0;
    { const double xc = clip(x); if (__ballot(valid && xc != x) == 0) return 1; x = xc; }
    if (valid) kf[tid] = x;
    wave_sync();
    const double qu = valid ? qu_[tid] : 0.0;
    double qm = 0.0;
    if (valid) for (int j = 0; j < m; ++j) qm = fmax(qm, fabs(Quu[j * m + tid] + (j == tid ? mu : 0.0)));
    const double qmax = wave_max(qm), qumax = wave_max(fabs(qu));
    unsigned long long prev = 0, factored = 0; bool have_prev = false, have_factor = false, prev_full = false;
    double rinv = 1.0;
    for (;;) {
        double g = 0.0;                                             // g = qu + Qreg x (Quu is symmetric: column tid is read, consecutive lanes consecutive addresses)
        if (valid) {
            double s = mu * x;
#pragma unroll 2
            for (int j = 0; j < m; ++j) s = fma(Quu[j * m + tid], kf[j], s);
            g = qu + s;
        }
        set = __ballot(valid && ((x <= lo && g > 0.0) || (x >= hi && g < 0.0)));
        const bool cl = set >> tid & 1;
        const int nfree = m - __popcll(set);
        const double gfree = wave_max(valid && !cl ? fabs(g) : 0.0), xmax = wave_max(fabs(x));
        if (nfree == 0 || (have_prev && set == prev && prev_full) || gfree <= 64.0 * 0x1p-52 * fmax(qumax, qmax * xmax)) break;
        if (it == 64) return -1;
        ++it;
        if (!box_factor(Quu, L, m, mu, set, tid, rinv)) return -1;
        factored = set; have_factor = true;
        const double d = box_solve(L, m, tid, rinv, valid && !cl ? -g : 0.0);
        double step = 1.0, xt = x, xu = x; bool accepted = false;
        for (int trial = 0; trial < 40 && !accepted; ++trial) {
            xu = fma(step, d, x); xt = clip(xu);
            const double dx = valid ? xt - x : 0.0;
            if (valid) dl[tid] = dx;
            wave_sync();
            double qd = 0.0;
            if (valid) {
                qd = mu * dx;
#pragma unroll 2
                for (int j = 0; j < m; ++j) qd = fma(Quu[j * m + tid], dl[j], qd);
            }
            wave_sync();
            const double gd = wave_add(g * dx), dqd = wave_add(dx * qd);          // f(x+) - f(x) = g' dx + 1/2 dx' Qreg dx
            accepted = gd + 0.5 * dqd <= 0.1 * gd;
            if (!accepted) step *= 0.5;
        }
        if (!accepted) return -1;
        prev = set; have_prev = true;
        prev_full = step == 1.0 && __ballot(valid && xt != xu) == 0;
        x = xt;
        if (valid) kf[tid] = x;
        wave_sync();
    }
    if (!have_factor || factored != set) { if (!box_factor(Quu, L, m, mu, set, tid, rinv)) return -1; }
    return 2;
}

// ---- the constraint rows of a stage (the AlArgs variant): acc += G' diag(w) G over the entries rc, q += G' y, G = [Cx Cu] (nc x N; columns >= cols count as zero:
// the terminal stage has cols = n), R rows at a time through the row buffers: Fb = G, Tb = diag(w) G, the accumulator loop of the sweep; q[j] is lane j's.  A row
// with w = y = 0 is not loaded; a block without a live row is skipped with its barriers.  That decision is the workgroup's: lane l of EVERY wavefront reads w, y of
// row i0 + l and the ballot gives each wavefront the same mask (one load per 64 rows, not one per row).  w0, y0: lane l's w, y of row l (rows < 64) when the caller
// has them already (have0: the sweep loads them a step ahead, so that their latency is not the step's).  Ends behind a barrier whenever it wrote to Fb, Tb ----
template <class TIO, int NQ>
__device__ __forceinline__ void al_rows(const TIO* Cx, const TIO* Cu, const TIO* wg, const TIO* yg, int nc, int n, int m, int cols, const int (&rc)[NQ], double (&acc)[NQ],
                                        double* Fb, double* Tb, double* q, int tid, bool have0, double w0, double y0) {
    const int N = n + m;
    for (int c0 = 0; c0 < nc; c0 += 64) {
        const int il = c0 + (tid & 63);
        double wl = w0, yl = y0;
        if (!(have0 && c0 == 0)) { wl = (double)wg[il < nc ? il : 0]; yl = (double)yg[il < nc ? il : 0]; }
        const unsigned long long live64 = __ballot(il < nc && !(wl == 0.0 && yl == 0.0));
        for (int i0 = c0; i0 < nc && i0 < c0 + 64; i0 += R) {
            const unsigned live = (unsigned)(live64 >> (i0 - c0)) & 0xffffu;
            if (live == 0) continue;
            for (int o = tid; o < R * N; o += THREADS) {
                const int kk = o / N, j = o - kk * N, i = i0 + kk;
                double g = 0.0, wi = 0.0;
                if ((live >> kk & 1) && j < cols) {
                    wi = (double)wg[i];
                    g = j < n ? (double)Cx[(size_t)i * n + j] : Cu ? (double)Cu[(size_t)i * m + (j - n)] : 0.0;
                }
                Fb[o] = g; Tb[o] = wi * g;
            }
            __syncthreads();
#pragma unroll
            for (int qq = 0; qq < NQ; ++qq) {
                int w = rc[qq]; DJ_OPAQUE(w);
                if (w >= 0) {
                    const double* const fr = Fb + (w >> 16); const double* const tc = Tb + (w & 0xffff);
                    double s = acc[qq];
#pragma unroll 4
                    for (int kk = 0; kk < R; ++kk) s = fma(fr[kk * N], tc[kk * N], s);
                    acc[qq] = s;
                }
            }
            for (int j = tid; j < cols; j += THREADS) {
                double s = q[j];
#pragma unroll 4
                for (int kk = 0; kk < R; ++kk) if (live >> kk & 1) s = fma((double)yg[i0 + kk], Fb[kk * N + j], s);
                q[j] = s;
            }
            __syncthreads();
        }
    }
}

// A_ = BoxArgs<TIO>: the control-limited variant (BOX; every difference sits behind `if constexpr (BOX)`: the instantiations over Args<TIO> keep their instructions)
// A_ = AlArgs<TIO>: the constrained variant (AL, with BOX; every difference behind `if constexpr (AL)`: the instantiations over Args and BoxArgs keep theirs)
template <class TIO, int NQ, class A_ = Args<TIO>>
__global__ void __launch_bounds__(THREADS) riccati_kernel(const A_ a) {
    constexpr bool AL = std::is_same<A_, AlArgs<TIO>>::value;
    constexpr bool BOX = AL || std::is_same<A_, BoxArgs<TIO>>::value;
    extern __shared__ __align__(16) double lds_[];
    const int H = a.H, B = a.B, n = a.n, nu = a.nu, m = a.m, N = n + m, b = (int)blockIdx.x, tid = (int)threadIdx.x;
    const int nV = n * (n + 1) / 2, ne = N * (N + 1) / 2;
    const TIO* const Ag = DJ_GLOBAL_PTR(const TIO, a.A); const TIO* const Bg = DJ_GLOBAL_PTR(const TIO, a.Bm);
    const TIO* const lxg = DJ_GLOBAL_PTR(const TIO, a.lx); const TIO* const lug = DJ_GLOBAL_PTR(const TIO, a.lu);
    const TIO* const lxxg = DJ_GLOBAL_PTR(const TIO, a.lxx); const TIO* const luug = DJ_GLOBAL_PTR(const TIO, a.luu); const TIO* const luxg = DJ_GLOBAL_PTR(const TIO, a.lux);
    const int* const status = DJ_GLOBAL_PTR(const int, a.status);
    TIO* const Kg = DJ_GLOBAL_PTR(TIO, a.K); TIO* const kffg = DJ_GLOBAL_PTR(TIO, a.kff);
    // LDS: Vp (packed Vxx) / K | row buffers Fb, Tb / Y (Qux), Quu, L | Vx, q = [Qx; Qu], kff, g, t, the flag
    double* const Vp = lds_; double* const K_ = lds_;
    double* const r1 = lds_ + nV;
    double* const Fb = r1; double* const Tb = r1 + R * N;
    double* const Y = r1; double* const Quu = r1 + m * n; double* const L = Quu + m * m;
    double* const Vx = r1 + ((2 * R * N > m * n + 2 * m * m) ? 2 * R * N : m * n + 2 * m * m);
    double* const qv = Vx + n; double* const kf = qv + N; double* const g_ = kf + m; double* const t_ = g_ + m;
    int* const flag = reinterpret_cast<int*>(t_ + m);
    unsigned long long* const clamped = reinterpret_cast<unsigned long long*>(t_ + m + 1);      // (BOX) the clamped set of the step
    double* const dl = t_ + m + 8;                                                               // (BOX) [m]: the trial step of the QP
    const double mu = a.mu ? (double)DJ_GLOBAL_PTR(const TIO, a.mu)[b] : 0.0;

    // the entries of Q this lane owns: (row << 16 | column), row >= column; -1: none.  (Every use below goes through DJ_OPAQUE: what is derived from an entry -- a
    // dozen addresses -- is then computed where it is used, not hoisted out of the step loop into registers that live for the whole launch.)
    int rc[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const int e = tid + q * THREADS;
        int r = (int)((sqrtf(8.0f * (float)e + 1.0f) - 1.0f) * 0.5f);
        while (r * (r + 1) / 2 > e) --r;
        while ((r + 1) * (r + 2) / 2 <= e) ++r;
        rc[q] = e < ne ? (r << 16 | (e - r * (r + 1) / 2)) : -1;
    }

    // the value function behind the last step
    {
        const size_t kb = (size_t)H * B + b;
        for (int e = tid; e < n * n; e += THREADS) {
            const int r = e / n, c = e - r * n;
            if (c <= r) Vp[r * (r + 1) / 2 + c] = 0.5 * ((double)lxxg[kb * n * n + e] + (double)lxxg[kb * n * n + (size_t)c * n + r]);
        }
        for (int i = tid; i < n; i += THREADS) Vx[i] = (double)lxg[kb * n + i];
    }
    double dV0 = 0.0, dV1 = 0.0;          // (lane 0's)
    __syncthreads();
    if constexpr (AL) {
        // the terminal rows: Vxx += sum_i w_i Cx_H[i]' Cx_H[i], Vx += sum_i y_i Cx_H[i] over the live rows, i ascending; the owner of a packed entry takes its own sum
        if (a.nc > 0) {
            const size_t kb = (size_t)H * B + b;
            double acc[NQ];
#pragma unroll
            for (int q = 0; q < NQ; ++q) { int w = rc[q]; DJ_OPAQUE(w); acc[q] = (w >= 0 && (w >> 16) < n) ? Vp[tid + q * THREADS] : 0.0; }
            al_rows<TIO, NQ>(DJ_GLOBAL_PTR(const TIO, a.Cx) + (a.shared ? (size_t)0 : kb * a.nc * n), nullptr, DJ_GLOBAL_PTR(const TIO, a.w) + kb * a.nc,
                             DJ_GLOBAL_PTR(const TIO, a.y) + kb * a.nc, a.nc, n, m, n, rc, acc, r1, r1 + R * N, Vx, tid, false, 0.0, 0.0);
#pragma unroll
            for (int q = 0; q < NQ; ++q) { int w = rc[q]; DJ_OPAQUE(w); if (w >= 0 && (w >> 16) < n) Vp[tid + q * THREADS] = acc[q]; }
            __syncthreads();
        }
    }

    TIO w_next = (TIO)0, y_next = (TIO)0;      // (AL) lane l of every wavefront: w, y of row l (rows < 64) of the step to come, loaded a step ahead
    (void)w_next; (void)y_next;
    if constexpr (AL) {
        if (a.nc > 0) {
            const size_t o = ((size_t)(H - 1) * B + b) * a.nc + ((tid & 63) < a.nc ? (tid & 63) : 0);
            w_next = DJ_GLOBAL_PTR(const TIO, a.w)[o]; y_next = DJ_GLOBAL_PTR(const TIO, a.y)[o];
        }
    }
    for (int k = H - 1; k >= 0; --k) {
        const size_t kb = (size_t)k * B + b;
        const bool failed = status != nullptr && status[kb] != 0;
        const TIO* const Ak = Ag + kb * n * n; const TIO* const Bk = Bg + kb * n * nu + a.act_off;
        auto F = [&](int i, int j) { return (double)(j < n ? Ak[(size_t)i * n + j] : Bk[(size_t)i * nu + (j - n)]); };
        double acc[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            int w = rc[q]; DJ_OPAQUE(w);
            const int r = w >> 16, c = w & 0xffff;
            double v = 0.0;
            if (w >= 0) {
                if (r < n) v = 0.5 * ((double)lxxg[kb * n * n + (size_t)r * n + c] + (double)lxxg[kb * n * n + (size_t)c * n + r]);
                else if (c < n) v = luxg ? (double)luxg[kb * m * n + (size_t)(r - n) * n + c] : 0.0;
                else v = 0.5 * ((double)luug[kb * m * m + (size_t)(r - n) * m + (c - n)] + (double)luug[kb * m * m + (size_t)(c - n) * m + (r - n)]);
            }
            acc[q] = v;
        }
        for (int j = tid; j < N; j += THREADS) qv[j] = j < n ? (double)lxg[kb * n + j] : (double)lug[kb * m + (j - n)];
        if (!failed) {
            for (int k0 = 0; k0 <= n; k0 += R) {
                for (int o = tid; o < R * N; o += THREADS) {
                    const int kk = o / N, j = o - kk * N;
                    Fb[o] = k0 + kk < n ? F(k0 + kk, j) : 0.0;
                }
                for (int o = tid; o < (R / RB) * N; o += THREADS) {
                    const int gq = o / N, j = o - gq * N, kr0 = k0 + gq * RB;
                    double s[RB];
#pragma unroll
                    for (int u = 0; u < RB; ++u) s[u] = 0.0;
                    if (kr0 <= n) {
#pragma unroll 2
                        for (int i = 0; i < n; ++i) {                    // (eight loads in flight instead of two: 181 VGPRs instead of 127, two workgroups per CU instead of four, Ant 5.5 ms instead of 3.2)
                            const double f = F(i, j);
#pragma unroll
                            for (int u = 0; u < RB; ++u) {
                                const int kr = kr0 + u;
                                const double v = kr < n ? Vp[kr >= i ? kr * (kr + 1) / 2 + i : i * (i + 1) / 2 + kr] : kr == n ? Vx[i] : 0.0;
                                s[u] = fma(v, f, s[u]);
                            }
                        }
                    }
#pragma unroll
                    for (int u = 0; u < RB; ++u) Tb[(gq * RB + u) * N + j] = kr0 + u <= n ? s[u] : 0.0;      // (a row past the last: 0, not 0 * F)
                }
                __syncthreads();
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    int w = rc[q]; DJ_OPAQUE(w);
                    if (w >= 0) {
                        const double* const fr = Fb + (w >> 16); const double* const tc = Tb + (w & 0xffff);
                        double s = acc[q];
#pragma unroll 4
                        for (int kk = 0; kk < R; ++kk) s = fma(fr[kk * N], tc[kk * N], s);
                        acc[q] = s;
                    }
                }
                if (k0 <= n && n < k0 + R) for (int j = tid; j < N; j += THREADS) qv[j] += Tb[(n - k0) * N + j];       // the row of Vx: Qx, Qu
                __syncthreads();
            }
        }
        if constexpr (AL) {
            // Q += G' diag(w) G, q += G' y over the live rows of the step (al_rows) -- also at a failed step: its cost terms stand
            if (a.nc > 0) {
                const double w_now = (double)w_next, y_now = (double)y_next;
                if (k > 0) {
                    const size_t o = (kb - B) * a.nc + ((tid & 63) < a.nc ? (tid & 63) : 0);
                    w_next = DJ_GLOBAL_PTR(const TIO, a.w)[o]; y_next = DJ_GLOBAL_PTR(const TIO, a.y)[o];
                }
                al_rows<TIO, NQ>(DJ_GLOBAL_PTR(const TIO, a.Cx) + (a.shared ? (size_t)0 : kb * a.nc * n),
                                 a.Cu ? DJ_GLOBAL_PTR(const TIO, a.Cu) + (a.shared ? (size_t)0 : kb * a.nc * m) : nullptr,
                                 DJ_GLOBAL_PTR(const TIO, a.w) + kb * a.nc, DJ_GLOBAL_PTR(const TIO, a.y) + kb * a.nc, a.nc, n, m, N, rc, acc, Fb, Tb, qv, tid, true, w_now, y_now);
            }
        }
        // Qux, Quu leave the registers
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            int w = rc[q]; DJ_OPAQUE(w);
            const int r = (w >> 16) - n, c = w & 0xffff;
            if (w >= 0 && r >= 0) {
                if (c < n) Y[r * n + c] = acc[q];
                else { Quu[r * m + (c - n)] = acc[q]; Quu[(c - n) * m + r] = acc[q]; }
            }
        }
        __syncthreads();
        // Qreg = L L^T: wavefront 0, lane = row
        double lo_ = -__builtin_huge_val(), hi_ = __builtin_huge_val();     // (BOX) lane i of wavefront 0: the limits of kff_i, lo[b][i] - U[k][b][act_off + i] and hi likewise
        if (tid < 64) {
            bool ok = true, empty = false;
            if constexpr (BOX) {
                if (tid < m) {
                    double u;
                    if constexpr (AL) u = a.U ? (double)DJ_GLOBAL_PTR(const TIO, a.U)[kb * nu + a.act_off + tid] : 0.0;      // (null only without limits)
                    else u = (double)DJ_GLOBAL_PTR(const TIO, a.U)[kb * nu + a.act_off + tid];
                    if (a.lo) lo_ = (double)DJ_GLOBAL_PTR(const TIO, a.lo)[(size_t)b * m + tid] - u;
                    if (a.hi) hi_ = (double)DJ_GLOBAL_PTR(const TIO, a.hi)[(size_t)b * m + tid] - u;
                }
                empty = __ballot(!(lo_ <= hi_)) != 0; ok = !empty;                               // (an empty or NaN box: the code is -(k + 1), nothing is factored)
            }
            for (int j = 0; j < (BOX && !ok ? 0 : m); ++j) {
                double s = 0.0;
                if (tid < m && tid >= j) {
                    s = Quu[tid * m + j] + (tid == j ? mu : 0.0);
#pragma unroll 2
                    for (int p = 0; p < j; ++p) s = fma(-L[tid * m + p], L[j * m + p], s);
                }
                const double d = __shfl(s, j);
                if (!(d > 0.0) || !(d < __builtin_huge_val())) { ok = false; break; }
                const double rd = sqrt(d);
                if (tid < m && tid >= j) L[tid * m + j] = tid == j ? rd : s / rd;
                wave_sync();
            }
            if (tid == 0) *flag = ok ? 1 : (BOX && empty) ? -1 : 0;
        }
        __syncthreads();
        if (BOX ? *flag <= 0 : *flag == 0) {
        failed:     // (BOX: a failed QP comes here from below; the code is the flag's)
            // steps <= k and the value function: zeros; the steps above keep what was computed
            for (int kz = 0; kz <= k; ++kz) {
                const size_t kzb = (size_t)kz * B + b;
                for (int e = tid; e < m * n; e += THREADS) Kg[kzb * m * n + e] = (TIO)0;
                for (int i = tid; i < m; i += THREADS) kffg[kzb * m + i] = (TIO)0;
                if constexpr (BOX) if (tid == 0) { if (a.active) a.active[kzb] = 0; if (a.iters) a.iters[kzb] = 0; }
            }
            if (a.dV && tid < 2) a.dV[(size_t)b * 2 + tid] = (TIO)0;
            if (a.Vx) for (int i = tid; i < n; i += THREADS) a.Vx[(size_t)b * n + i] = (TIO)0;
            if (a.Vxx) for (int e = tid; e < n * n; e += THREADS) a.Vxx[(size_t)b * n * n + e] = (TIO)0;
            if (tid == 0) a.fail[b] = (BOX && *flag < 0) ? -(k + 1) : k + 1;
            return;
        }
        // K = -Qreg^-1 Qux, kff = -Qreg^-1 Qu: one lane per right-hand side, in place (K over the dead Vxx)
        for (int c = tid; c <= n; c += THREADS) {
            double* const x = c < n ? K_ + c : kf; const int ld = c < n ? n : 1;
            for (int i = 0; i < m; ++i) {
                double s = c < n ? Y[i * n + c] : qv[n + i];
#pragma unroll 2
                for (int p = 0; p < i; ++p) s = fma(-L[i * m + p], x[p * ld], s);
                x[i * ld] = s / L[i * m + i];
            }
            for (int i = m - 1; i >= 0; --i) {
                double s = x[i * ld];
#pragma unroll 2
                for (int p = i + 1; p < m; ++p) s = fma(-L[p * m + i], x[p * ld], s);
                x[i * ld] = s / L[i * m + i];
            }
            for (int i = 0; i < m; ++i) x[i * ld] = -x[i * ld];
        }
        __syncthreads();
        if constexpr (BOX) {
            // kf holds -Qreg^-1 Qu and K_ the unconstrained gains, both exactly riccati_kernel's.  Wavefront 0 clips kf; where that changes nothing the step is
            // done (no iteration, nothing clamped), otherwise it solves the QP, leaves the factor masked by the clamped set in L, and the gains are solved again
            if (tid < 64) {
                unsigned long long set = 0; int it = 0;
                const int code = box_qp(Quu, L, kf, dl, qv + n, m, mu, lo_, hi_, tid, set, it);       // -1: failed, 1: nothing clipped, 2: solved, L is the masked factor
                if (tid == 0) {
                    *flag = code; *clamped = set;
                    if (code > 0) { if (a.active) a.active[kb] = (long long)set; if (a.iters) a.iters[kb] = it; }
                }
            }
            __syncthreads();
            if (*flag < 0) goto failed;
            if (*flag == 2) {
                const unsigned long long set = *clamped;
                for (int c = tid; c < n; c += THREADS) {
                    double* const x = K_ + c;
                    for (int i = 0; i < m; ++i) {
                        double s = (set >> i & 1) ? 0.0 : Y[i * n + c];
#pragma unroll 2
                        for (int p = 0; p < i; ++p) s = fma(-L[i * m + p], x[p * n], s);
                        x[i * n] = s / L[i * m + i];
                    }
                    for (int i = m - 1; i >= 0; --i) {
                        double s = x[i * n];
#pragma unroll 2
                        for (int p = i + 1; p < m; ++p) s = fma(-L[p * m + i], x[p * n], s);
                        x[i * n] = s / L[i * m + i];
                    }
                    for (int i = 0; i < m; ++i) x[i * n] = (set >> i & 1) ? 0.0 : -x[i * n];
                }
                __syncthreads();
            }
        }
        // t = Quu kff, g = t / 2 + Qu, Y = Quu K / 2 + Qux; the gains leave
        for (int i = tid; i < m; i += THREADS) {
            double s = 0.0;
#pragma unroll 2
            for (int j = 0; j < m; ++j) s = fma(Quu[i * m + j], kf[j], s);
            t_[i] = s; g_[i] = 0.5 * s + qv[n + i];
            kffg[kb * m + i] = (TIO)kf[i];
        }
        for (int e = tid; e < m * n; e += THREADS) {
            const int i = e / n, c = e - i * n;
            double s = 0.0;
#pragma unroll 2
            for (int j = 0; j < m; ++j) s = fma(Quu[i * m + j], K_[j * n + c], s);
            Y[e] = 0.5 * s + Y[e];
            Kg[kb * m * n + e] = (TIO)K_[e];
        }
        __syncthreads();
        if (tid == 0) {
            double s0 = 0.0, s1 = 0.0;
            for (int i = 0; i < m; ++i) { s0 = fma(kf[i], qv[n + i], s0); s1 = fma(kf[i], t_[i], s1); }
            dV0 += s0; dV1 += 0.5 * s1;
        }
        double vx_new = 0.0;                                    // (n <= 110 < THREADS: one entry per lane)
        if (tid < n) {
            double s = qv[tid];
#pragma unroll 2
            for (int i = 0; i < m; ++i) s = fma(Y[i * n + tid], kf[i], fma(K_[i * n + tid], g_[i], s));
            vx_new = s;
        }
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            int w = rc[q]; DJ_OPAQUE(w);
            const int r = w >> 16, c = w & 0xffff;
            if (w >= 0 && r < n) {
                double s = acc[q];
#pragma unroll 2
                for (int i = 0; i < m; ++i) s = fma(K_[i * n + r], Y[i * n + c], fma(Y[i * n + r], K_[i * n + c], s));
                acc[q] = s;
            }
        }
        __syncthreads();
        if (tid < n) Vx[tid] = vx_new;
#pragma unroll
        for (int q = 0; q < NQ; ++q) { int w = rc[q]; DJ_OPAQUE(w); if (w >= 0 && (w >> 16) < n) Vp[tid + q * THREADS] = acc[q]; }       // (the packed index of (r, c), r < n, is the entry's own)
        __syncthreads();
    }
    if (tid == 0) {
        a.fail[b] = 0;
        if (a.dV) { a.dV[(size_t)b * 2] = (TIO)dV0; a.dV[(size_t)b * 2 + 1] = (TIO)dV1; }
    }
    if (a.Vx) for (int i = tid; i < n; i += THREADS) a.Vx[(size_t)b * n + i] = (TIO)Vx[i];
    if (a.Vxx) for (int e = tid; e < n * n; e += THREADS) {
        const int r = e / n, c = e - r * n;
        a.Vxx[(size_t)b * n * n + e] = (TIO)Vp[r >= c ? r * (r + 1) / 2 + c : c * (c + 1) / 2 + r];
    }
}
#endif

}  // namespace riccati
}  // namespace dj
