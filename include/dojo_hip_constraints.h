/*
 * dojo_hip_constraints.h -- constrained iLQR on the device, the entries of libdojo_hip.so that came after dojo_hip.h, dojo_hip_trajopt.h and dojo_hip_limits.h:
 * the Riccati backward pass with the augmented-Lagrangian (AL) terms of linearized stage constraints added to the step's quadratic model inside the kernel.
 *
 * This is the backward pass IterativeLQR runs under its augmented-Lagrangian outer loop (the reference's examples/trajectory_optimization give it a terminal goal
 * constraint and, some, state or control bounds): for constraint rows c(x, u) with Jacobian G = [Cx Cu], row weights w and multiplier estimates y the stage cost
 * gains  G' diag(w) G  in its Hessian and  G' y  in its gradient.  They are never formed in memory: the kernel feeds blocks of 16 rows of G through the loop
 * that accumulates Q = l + F' (Vxx F) in registers.
 */
#ifndef DOJO_HIP_CONSTRAINTS_H
#define DOJO_HIP_CONSTRAINTS_H

#include "dojo_hip_limits.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The linearized constraints of every stage, n = 2 nu, na the driven inputs of the DojoRiccati record, in the handle dtype.  Device pointers for the _dev entry,
 * host pointers for the other.  The struct is host memory, read during the call.
 *     Cx  [H+1][B][nc][n],  or [nc][n]  when shared != 0      the state Jacobian of the rows
 *     Cu  [H][B][nc][na],   or [nc][na] when shared != 0      the control Jacobian; NULL: zeros
 *     w   [H+1][B][nc]      the weight of a row: the penalty on an active row, 0 on an inactive or absent one
 *     y   [H+1][B][nc]      the multiplier estimate of the row, lambda + w c
 * nc = 0 is legal; Cx, Cu, w, y may then be NULL.  The library knows nothing about equalities, inequalities or active sets: that is elementwise work for the caller. */
typedef struct DojoStageConstraints {
    const void *Cx, *Cu, *w, *y;
    int32_t nc, shared;
} DojoStageConstraints;

/* ---- The constrained backward pass (csrc/dojo_riccati.hpp, riccati_kernel over AlArgs) ----
 * Per environment b, in fp64, G_k = [Cx_k Cu_k] (nc x (n + na)), row i of step k LIVE unless w[k][b][i] == 0 and y[k][b][i] == 0:
 *     Vxx <- sym(lxx_H);  Vx <- lx_H                                             (dojo_riccati_dev)
 *     Vxx[r][c] = fma(Cx_H[i][r], w_i Cx_H[i][c], Vxx[r][c]),   Vx[j] = fma(y_i, Cx_H[i][j], Vx[j])       over the live rows i, ascending
 *     for k = H-1 .. 0:
 *         Qx, Qu, Qxx, Qux, Quu as in dojo_riccati_dev ("Batched iLQR", dojo_hip.h), a step with status != 0 counting its A_k, B_k as zero
 *         Q  += G_k' diag(w) G_k,   [Qx; Qu] += G_k' y         over the live rows, ascending, 16 at a time -- ALSO at a step with status != 0: a failed dynamics
 *                                                              step still has its cost terms
 *         the limits, the Cholesky, the box QP, the gains and the value update of dojo_riccati_box_dev (dojo_hip_limits.h), unchanged
 * A row that is not live is NOT LOADED: it contributes exact zeros and a NaN in its Cx / Cu is harmless; a block of 16 rows none of which is live costs two
 * scalar reads per row and nothing else.  A terminal-only constraint therefore costs nothing at the steps before the last.
 * dV is the model of the merit  M = J + sum lambda c + 1/2 sum w c^2  when y = lambda + w c: a dV[0] + a^2 dV[1] for the step length a.
 *
 * lim = NULL: no control limits (U may then be NULL too); with limits U is required, as in dojo_riccati_box_dev.
 * Outputs, failure codes and their zeros: those of dojo_riccati_box_dev.  A negative or NaN w is not examined on the device; it surfaces as a pivot failure or
 * not at all.  The host entry refuses it.
 *
 * No atomics.  Every sum runs in an order fixed by (n, na, nc) and by which rows are live: results are bit-identical from run to run and do not depend on B or
 * on the environment's place in the batch.  With nc = 0, or with all w = y = 0, every output is dojo_riccati_box_dev's bit for bit; with infinite or NULL limits
 * as well, dojo_riccati_dev's.  `shared` gives the bits of the same matrices replicated, Cu = NULL those of zeros.
 *
 * dojo_riccati_al_dev: device pointers, enqueued on `stream`, no synchronization.  dojo_riccati_al: host pointers, staged like the other host entries.
 * Refused before anything is launched, text on the handle: whatever dojo_riccati_dev refuses (with this entry's name); DOJO_ERR_INVALID: NULL con, nc < 0, nc > 0
 * with NULL Cx, w or y, NULL U with non-NULL lim; DOJO_ERR_UNSUPPORTED: the plan's LDS (dojo_riccati_box_dev's: the constraint blocks use the row buffers that
 * are there) over 65536 bytes, byte count in the text.  The host entry also reads the limits and w, y and refuses lo > hi, NaN limits, w < 0 and NaN in w or y
 * with DOJO_ERR_INVALID.
 *
 * Not part of it: second-order constraint terms, constraints evaluated on the device, per-row penalties (the caller's w already is one), a warm start of the
 * multipliers across calls, running the step lengths of a line search side by side.  (The last came later, as entries of their own:
 * include/dojo_hip_linesearch.h; its mode without a cost takes this loop's merit.)
 */
int dojo_riccati_al_dev(DojoHandle h, int32_t H, const DojoRiccati* r, const DojoControlLimits* lim /* NULL: no limits */,
                        const void* U /* [H][B][nu]; may be NULL iff lim is NULL */, const DojoStageConstraints* con,
                        int64_t* active /* [H][B] or NULL */, int32_t* qp_iters /* [H][B] or NULL */, void* stream);
int dojo_riccati_al(DojoHandle h, int32_t H, const DojoRiccati* r, const DojoControlLimits* lim, const void* U, const DojoStageConstraints* con,
                    int64_t* active, int32_t* qp_iters);

#ifdef __cplusplus
}
#endif
#endif
