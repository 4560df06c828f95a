/*
 * dojo_hip_linesearch.h -- the line search of iLQR on the device, the entries of libdojo_hip.so that came after dojo_hip.h, dojo_hip_trajopt.h, dojo_hip_limits.h
 * and dojo_hip_constraints.h: the step lengths of a line search rolled out side by side in ONE rollout, and ONE kernel that evaluates the costs of the trials,
 * applies the acceptance test, picks the first acceptable trial of every problem and gathers its trajectory.
 *
 * IterativeLQR walks the step lengths 1, 1/2, 1/4, .. one after another and stops at the first that passes an Armijo test.  T trials as one batch of T P
 * environments cost less than T forward passes (measured: 1.1 .. 1.9 passes for 8 trials of 64 .. 512 problems), and the host reads nothing back:
 * the whole iteration can be enqueued.  It pays when an iteration needs two or more step lengths.
 */
#ifndef DOJO_HIP_LINESEARCH_H
#define DOJO_HIP_LINESEARCH_H

#include "dojo_hip_constraints.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- The fan: T trials of P problems in one rollout (csrc/dojo_tracking.hpp, rollout_tracking_kernel over FanArgs) ----
 * The handle has batch B = T P.  Environment e = tr P + p is trial tr of problem p (trial-major: the P environments of a trial are contiguous in every output).
 *     per PROBLEM, read at p = e mod P:   x0 [P][n], Ubar [H][P][nu], Xbar [H+1][P][n], K [H][P][na][n], kff [H][P][na], lo / hi [P][na]
 *     per ENVIRONMENT:                    alpha [T][P] (= [B]: every problem may have its own ladder of step lengths), X [H+1][B][n], U_out [H][B][nu], status [H][B]
 * The law is that of dojo_rollout_minimal_box_dev (dojo_hip_limits.h), the same fp64 arithmetic in the same order, clamped in front of the one rounding; with
 * lim = NULL it is that of dojo_rollout_minimal_dev (dojo_hip_trajopt.h).  X[0][tr P + p] = x0[p].
 *
 * X, U_out and status are, bit for bit, what dojo_rollout_minimal_box_dev (lim = NULL: dojo_rollout_minimal_dev) returns on the same handle with every reference
 * member repeated T times along the batch axis.  Same lanes, no LDS, no atomics: bit-identical from run to run, independent of the environment groups
 * (dojo_set_groups; a group may begin and end inside a trial), of B and of the environment's place in the batch.
 *
 * dojo_rollout_minimal_fan_dev: device pointers, enqueued on `stream`, no synchronization.  dojo_rollout_minimal_fan: host pointers, [P]-sized inputs and [B]-sized
 * outputs staged like the other host entries.  The structs are host memory, read during the call.
 * Refused before anything is launched, text on the handle, outputs untouched: whatever dojo_rollout_minimal_dev refuses (with this entry's name);
 * DOJO_ERR_INVALID: T < 1, B mod T != 0, A or Bm given (the fan does not record Jacobians); the host entry also lo > hi and NaN limits.
 */
int dojo_rollout_minimal_fan_dev(DojoHandle h, int32_t H, int32_t T, const DojoTracking* t, const DojoControlLimits* lim /* may be NULL */, void* stream);
int dojo_rollout_minimal_fan(DojoHandle h, int32_t H, int32_t T, const DojoTracking* t, const DojoControlLimits* lim /* may be NULL */);

/* ---- The selection (csrc/dojo_linesearch.hpp, linesearch_select_kernel) ----
 * The quadratic cost of ilqr.QuadraticCost, shared by the problems, in the handle dtype: Q [n][n], R [na][na], Qf [n][n], goal [n] -- or [P][n] with
 * goal_per_problem != 0.  Device pointers for the _dev entry, host pointers for the other. */
typedef struct DojoQuadraticCost { const void *Q, *R, *Qf, *goal; int32_t goal_per_problem; } DojoQuadraticCost;

/* The handle is the fan's: P = B / T.  Arrays are in the handle dtype unless a type is named; the cost values are double whatever the handle dtype (a
 * comparison of costs never passes through an fp32 rounding).
 *     X [H+1][T P][n], U [H][T P][nu], status [H][T P] (int32; NULL: all solved)     the trials, as the fan leaves them
 *     alpha [T][P], dV [P][2]                                                         the step lengths; dojo_riccati*_dev's dV
 *     ok [P] (int32) or NULL                                                          0: this problem accepts nothing (a failed backward pass or linearization)
 *     Xcur [H+1][P][n], Ucur [H][P][nu]                                               the trajectory the pass was taken around
 *     J0 [P] (double)                                                                 its cost; NULL with a cost: computed from Xcur, Ucur by the same code
 *     J_trial [T][P] (double)                                                         OUTPUT with a cost, INPUT without
 *     J_cur [P] (double) or NULL, J_acc [P] (double)                                  outputs: J0 as used; the cost of the accepted trial, or J0
 *     choice [P] (int32), alpha_acc [P]                                               outputs: the accepted trial or -1; its step length or 0
 *     X_new [H+1][P][n], U_new [H][P][nu]                                             outputs, each may be NULL: the accepted trial's columns, or Xcur / Ucur
 * Per problem p, e = tr P + p:
 *     with a cost:   J_tr = sum_{k<H} (1/2 d_k' Q d_k + 1/2 u_k' R u_k) + 1/2 d_H' Qf d_H,   d_k = (double)X[k][e] - (double)goal,  u_k = U[k][e][act_off .. act_off + na - 1]
 *                    in fp64: lane j takes the rows j, j + 64, .. of every step's products -- r = sum_c M[j][c] d_c, then d_j r, with fma, c and k ascending, the R rows
 *                    of a step behind its Q rows --, the 64 partial sums meet in a fixed order, the result is halved.  The order depends on n, na and H alone.
 *     without:       J_tr = J_trial[tr][p] and J0 as given (arbitrary cost objects; the merit of an augmented Lagrangian)
 *     trial tr is ACCEPTABLE when  ok[p] != 0,  every status[k][e] == 0,  J_tr <= J0 + c1 (a dV[p][0] + a a dV[p][1])  in fp64 with a = alpha[tr][p],  and J_tr is not NaN
 *     choice[p] = the FIRST acceptable tr in ascending order (first, not best), -1 when none is
 *     accepted:  alpha_acc, J_acc = that trial's;  X_new[:, p], U_new[:, p] = exact copies of that trial's columns
 *     none:      alpha_acc = 0,  J_acc = J0;       X_new, U_new = copies of Xcur, Ucur
 * Every element of every non-NULL output is written.
 *
 * One workgroup per problem, its wavefronts over the trials; the T costs and flags meet in LDS, one ascending scan chooses, all lanes copy.  No atomics:
 * bit-identical from run to run, independent of P and of where a problem sits.
 *
 * dojo_linesearch_select_dev: device pointers, enqueued on `stream`, no synchronization with the host; like the other _dev entries it first makes `stream` wait
 * (an event wait on the device) for asynchronous steps of the handle's environment groups that are still in flight, which may be writing the trials.  dojo_linesearch_select: host pointers, staged like the other host entries.
 * Refused before anything is launched, text on the handle, outputs untouched -- DOJO_ERR_INVALID: NULL handle or record; H < 1; T < 1, T > 64 (the LDS buffer
 * holds 64 trials) or B mod T != 0; NULL X, U, alpha, dV, Xcur, Ucur, choice, alpha_acc or J_acc; NULL J_trial; NULL J0 without a cost; with a cost, NULL Q, R, Qf or
 * goal; nu = 0, na < 1, act_off < 0 or act_off + na > nu; c1 not finite.
 *
 * Not part of it: constraints in the side-by-side driver (the mode without a cost is the hook), quadratization on the device, cost Hessians shared across the batch
 * in the Riccati kernel, skipping accepted environments inside a rollout, second-order dynamics terms, kinematic loops.
 */
typedef struct DojoLineSearch {
    const void *X, *U; const int32_t* status;
    const void *alpha, *dV;
    const int32_t* ok;
    const void *Xcur, *Ucur;
    const double* J0;
    double *J_trial, *J_cur, *J_acc;
    int32_t* choice; void *alpha_acc;
    void *X_new, *U_new;
    double c1; int32_t act_off, na;
} DojoLineSearch;
int dojo_linesearch_select_dev(DojoHandle h, int32_t H, int32_t T, const DojoQuadraticCost* cost /* may be NULL */, const DojoLineSearch* ls, void* stream);
int dojo_linesearch_select(DojoHandle h, int32_t H, int32_t T, const DojoQuadraticCost* cost /* may be NULL */, const DojoLineSearch* ls);

#ifdef __cplusplus
}
#endif
#endif
