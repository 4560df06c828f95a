/*
 * dojo_hip_limits.h -- control-limited iLQR on the device, the entries of libdojo_hip.so that came after dojo_hip.h and dojo_hip_trajopt.h: the Riccati backward
 * pass with a box-constrained QP per step, and the rollout in minimal coordinates with the clamped tracking law.
 *
 * This is control-limited DDP (Tassa, Mansard, Todorov: "Control-Limited Differential Dynamic Programming", ICRA 2014) on dojo_riccati_dev and
 * dojo_rollout_minimal_dev: the backward pass minimises the step's quadratic model over the box the limits leave around the current controls, the gain rows of
 * clamped inputs are zero, and the forward pass clamps.
 */
#ifndef DOJO_HIP_LIMITS_H
#define DOJO_HIP_LIMITS_H

#include "dojo_hip_trajopt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The limits of the m = na driven inputs act_off .. act_off + na - 1, per environment, constant over the horizon, in the handle dtype.  +-inf are allowed; a
 * NULL side is -inf / +inf.  Device pointers for the _dev entries, host pointers for the others.  The struct is host memory, read during the call. */
typedef struct DojoControlLimits { const void *lo, *hi; } DojoControlLimits;   /* [B][na] each, handle dtype, +-inf allowed, either may be NULL */

/* ---- The limited backward pass (csrc/dojo_riccati.hpp, riccati_kernel over BoxArgs) ----
 * Per environment b and step k = H-1 .. 0, in fp64.  Qx, Qu, Qxx, Qux, Quu are formed as in dojo_riccati_dev ("Batched iLQR", dojo_hip.h), Qreg = Quu + mu[b] I.
 *     lo' = (double)lo[b] - (double)U[k][b][act_off ..],  hi' = (double)hi[b] - (double)U[k][b][act_off ..]
 *     !(lo'_i <= hi'_i) for some i (NaN included):  fail[b] = -(k + 1), stop this environment
 *     Qreg = L L^T;  a pivot that is not > 0 or not finite:  fail[b] = k + 1, stop this environment      (dojo_riccati_dev's failure)
 *     kff = argmin_x  1/2 x' Qreg x + Qu' x   s.t.  lo' <= x <= hi'
 *     g   = Qu + Qreg kff;   clamped_i = (kff_i <= lo'_i and g_i > 0) or (kff_i >= hi'_i and g_i < 0);   free = not clamped
 *     K[free rows] = -Qreg[free, free]^-1 Qux[free rows];   K[clamped rows] = 0
 *     dV, Vx, Vxx: the formulas of dojo_riccati_dev, unchanged, with this kff and K
 * A clamped kff_i is lo'_i or hi'_i itself: rounded once to the handle dtype it is lo[b][i] - U[k][b][act_off + i] formed in fp64.
 *
 * The solver is projected Newton, on one wavefront, lane = row:
 *     x = clip(-Qreg^-1 Qu), the solve being dojo_riccati_dev's own.  If the clip changes no component the step is done: no iteration, nothing clamped, and K is
 *     dojo_riccati_dev's, bit for bit (the kernel solves K and kff exactly as dojo_riccati_dev does and looks at the limits afterwards; only a step whose start
 *     point is clipped runs the QP and solves K a second time, with the masked factor).
 *     Otherwise, per iteration:  g = Qu + Qreg x and the clamped set as above.  STOP when nothing is free, or when the set equals the previous iteration's and the
 *     previous step was a full step (s = 1) that clipped no component, or when max|g_free| <= 64 2^-52 max(max|Qu|, max|Qreg| max|x|).  Else factor Qreg with the
 *     clamped rows and columns replaced by the identity's (the Cholesky of the sweep; a bad pivot there is a failure of the QP), d_free = -Qreg_ff^-1 g_free,
 *     d_clamped = 0, and take the first s = 1, 1/2, .. (at most 40 trials) with
 *         f(x+) - f(x) <= 0.1 g' (x+ - x),     x+ = clip(x + s d),     f(x+) - f(x) evaluated as g' dx + 1/2 dx' Qreg dx,  dx = x+ - x.
 *     More than 64 iterations, no accepted s, or a bad pivot of the masked factor:  fail[b] = -(k + 1).
 *     The clamped set reported, and used for K, is the one of the last g.  qp_iters[k][b] counts the factorizations inside the loop.
 * The minimiser is unique; K is unique wherever the solution is strictly complementary (no clamped g_i = 0, no free x_i on a bound).
 *
 * Outputs: those of the DojoRiccati record; active[k][b] (bit i = input act_off + i clamped at step k) and qp_iters[k][b], each [H][B] or NULL.  Every element
 * of every output is written in every case.  A failed environment (fail[b] != 0, failure at step k) has zeros in K, kff, active and qp_iters of the steps <= k
 * and in dV, Vx, Vxx; the steps above k keep what was computed.  A step whose status is != 0 is not read (its A_k, B_k count as zero), as in dojo_riccati_dev.
 *
 * No atomics.  Every sum runs in an order fixed by (n, m) -- the two scalar sums of a trial step cross the 64 lanes in a fixed butterfly -- and the iteration count
 * depends on the environment's own data alone: results are bit-identical from run to run and do not depend on B or on the environment's place in the batch.
 * With infinite limits, NULL limits or limits that clip nothing, K, kff, dV, Vx, Vxx and fail are dojo_riccati_dev's bit for bit; active and qp_iters are 0.
 *
 * dojo_riccati_box_dev: device pointers, enqueued on `stream`, no synchronization.  dojo_riccati_box: host pointers, staged like the other host entries.
 * Refused before anything is launched, text on the handle: whatever dojo_riccati_dev refuses (with this entry's name); DOJO_ERR_INVALID: NULL lim or NULL U;
 * DOJO_ERR_UNSUPPORTED: the plan's LDS (dojo_riccati_dev's + na doubles) over 65536 bytes, byte count in the text.  The host entry also reads the limits and
 * refuses lo > hi and NaN with DOJO_ERR_INVALID; on the device entry those are the -(k + 1) code.
 */
int dojo_riccati_box_dev(DojoHandle h, int32_t H, const DojoRiccati* r, const DojoControlLimits* lim, const void* U /* [H][B][nu] */,
                         int64_t* active /* [H][B] or NULL: bit i = input act_off + i clamped */, int32_t* qp_iters /* [H][B] or NULL */, void* stream);
int dojo_riccati_box(DojoHandle h, int32_t H, const DojoRiccati* r, const DojoControlLimits* lim, const void* U, int64_t* active, int32_t* qp_iters);

/* ---- The clamped tracking law (csrc/dojo_tracking.hpp, rollout_tracking_kernel over BoxArgs) ----
 * dojo_rollout_minimal_dev with one change: for the driven inputs
 *     u[act_off + i] = min(max(Ubar[k][b][act_off + i] + a_i, (double)lo[b][i]), (double)hi[b][i])      in fp64, then rounded once
 * with a_i exactly as there; the inputs that are not driven are copied as there.  The limits are values of the handle dtype and rounding is monotone, so clamping
 * in front of the rounding equals clamping behind it: a driven input of U_out is inside [lo, hi] exactly.  A NaN limit is not looked at specially (the comparison
 * with it is false); the host entry refuses it.  X, status, A, Bm are, bit for bit, what dojo_step_minimal_dev / dojo_minimal_gradients_dev give at
 * (X[k], U_out[k]); with infinite or NULL limits every output is dojo_rollout_minimal_dev's bit for bit.  Same lanes, no LDS, no atomics: bit-identical from run
 * to run, independent of the environment groups, of B and of the environment's place in the batch.
 * Refused: whatever dojo_rollout_minimal_dev refuses (with this entry's name); DOJO_ERR_INVALID: NULL lim; the host entry also lo > hi and NaN limits.
 *
 * Not part of it: state constraints, time-varying limits, a warm start of the QP from the previous iteration's clamped set, limits on inputs that are not driven.
 * (The clamped law over T step lengths of a line search at once: include/dojo_hip_linesearch.h.)
 */
int dojo_rollout_minimal_box_dev(DojoHandle h, int32_t H, const DojoTracking* t, const DojoControlLimits* lim, void* stream);
int dojo_rollout_minimal_box(DojoHandle h, int32_t H, const DojoTracking* t, const DojoControlLimits* lim);

#ifdef __cplusplus
}
#endif
#endif
