/*
 * dojo_hip_trajopt.h -- the trajectory-optimization entries of libdojo_hip.so that came after the 74 of dojo_hip.h: rollouts in minimal coordinates
 * with a time-varying tracking controller, and the linearization along them.
 *
 * The reference's counterpart is simulate! driven through DojoEnvironments.step! (minimal state in, minimal state out: step_minimal_coordinates!,
 * src/simulation/step.jl:42-60) with a finite-horizon LQR or tracking controller u_k = ubar_k + K_k (x_k - xbar_k), and -- with A, Bm -- the
 * get_minimal_gradients! (src/gradients/state.jl:183-217) of every step: the forward pass and the linearization of IterativeLQR, each as ONE call.
 */
#ifndef DOJO_HIP_TRAJOPT_H
#define DOJO_HIP_TRAJOPT_H

#include "dojo_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The law, per environment b and step k = 0 .. H-1 (csrc/dojo_tracking.hpp).  n = 2 nu; the controller drives the m = na inputs act_off .. act_off + na - 1 as in
 * DojoPolicy.  All arrays are in the handle dtype.
 *     X[0]   = x0                                                       (copied)
 *     dx_j   = (double)X[k][b][j] - (double)Xbar[k][b][j]               from the ROUNDED X[k]; Xbar NULL: 0
 *     a_i    = fma(alpha[b], kff[k][b][i], sum_j K[k][b][i][j] dx_j)    fp64; alpha NULL: 1; kff NULL: 0; K NULL: 0 (Xbar is then not read)
 *     u      = Ubar[k][b];  u[act_off + i] += a_i                       rounded once -> U_out[k][b], read by step k (Ubar NULL: zeros)
 *     z      = minimal_to_maximal(X[k][b])                              from the ROUNDED X[k]: the step's input, as dojo_step_minimal_dev forms it
 *     z+     = step(z, u);  X[k+1][b] = maximal_to_minimal(z+)          rounded once
 *     optional: A[k][b] [n][n], Bm[k][b] [n][nu] = jx, ju of dojo_minimal_gradients_dev at (X[k], U_out[k]), in the handle's gradient mode
 * K [H][B][na][n] and kff [H][B][na] are exactly the outputs of dojo_riccati_dev; Xbar is [H+1][B][n] (row H is never read); alpha [B] is a step length per
 * environment, so that a line search needs no host value.  X is [H+1][B][n], U_out and Ubar [H][B][nu], status [H][B] (int32, may be NULL), A [H][B][n][n] and
 * Bm [H][B][n][nu] row-major (the record dojo_riccati_dev reads; both or neither).  What is recorded is what the controller saw: U_out[k] can be recomputed
 * from X[k] and the inputs alone.  A failed step is treated as the stepwise path treats it: the state is whatever the step leaves, status[k][b] != 0, and
 * nothing else is special.
 *
 * X, status, A and Bm equal, bit for bit, what H calls of dojo_step_minimal_dev / dojo_minimal_gradients_dev at (X[k], U_out[k]) give.  The sum over j is taken
 * by lane j over j, j + 64, ... ascending with fma, then over the 64 lanes in a fixed order: it depends on n alone.  No atomics: results are bit-identical from run
 * to run and do not depend on the number of environment groups (dojo_set_groups), on B or on where in the batch an environment sits.
 *
 * The environment groups of the handle run the H steps each at its own pace, with the controller between two steps on the group's stream: there is no
 * batch-wide join inside the call.  With A, Bm the batch is ONE group on the caller's stream (the Jacobian chain keeps 8.9 KB of scratch per lane, which the
 * runtime provides per hardware queue: one queue's worth, as in dojo_minimal_gradients_dev).  Afterwards the handle holds the last step's input and output state as after dojo_step_minimal_dev.
 * dojo_rollout_minimal_dev: device pointers, enqueued on `stream`, no synchronization.  dojo_rollout_minimal: host pointers, staged like the other host entries.
 * The struct is host memory, read during the call.
 *
 * Refused before anything is launched, text on the handle -- DOJO_ERR_INVALID: NULL handle or record; H < 1; NULL x0, X or U_out; nu = 0; na < 1, act_off < 0
 * or act_off + na > nu; exactly one of A, Bm given.  DOJO_ERR_UNSUPPORTED: a mechanism with a kinematic loop (as dojo_step_minimal_dev); with A, whatever the
 * recording rollouts refuse.  (The controller kernel keeps nothing in LDS: no shape is refused for its size.)
 * Not part of it: control limits / clamping (dojo_rollout_minimal_box_dev of include/dojo_hip_limits.h has them), costs on the device, running all step lengths of a line search side by side, reverse mode through the tracking
 * controller, contact observations, kinematic loops.  (The quadratic cost of a line search's trials and the step lengths side by side came later, as entries of
 * their own: include/dojo_hip_linesearch.h.) */
typedef struct DojoTracking {
    const void *x0, *Ubar, *Xbar, *K, *kff, *alpha;   /* [B][n] (required), [H][B][nu], [H+1][B][n], [H][B][na][n], [H][B][na], [B]; each of the last five may be NULL */
    void *X, *U_out;                                  /* [H+1][B][n], [H][B][nu]: required */
    int32_t* status;                                  /* [H][B] or NULL */
    void *A, *Bm;                                     /* [H][B][n][n], [H][B][n][nu] row-major: both or neither */
    int32_t act_off, na;
} DojoTracking;
int  dojo_rollout_minimal_dev(DojoHandle h, int32_t H, const DojoTracking* t, void* stream);
int  dojo_rollout_minimal(DojoHandle h, int32_t H, const DojoTracking* t);

#ifdef __cplusplus
}
#endif
#endif
