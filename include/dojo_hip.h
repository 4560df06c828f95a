/*
 * dojo_hip.h -- C ABI of libdojo_hip.so: the MI355X-native batched replacement for
 * Dojo.jl's per-timestep contact-implicit forward/backward path.
 *
 * The reference (Dojo.jl, 100 % Julia) has no FFI for this path; the seams this
 * library replaces are plain Julia method calls on a mutable `Mechanism`:
 *
 *   dojo_create        <- Mechanism(origin, bodies, joints, contacts; timestep, input_scaling, gravity)
 *                         src/mechanism/constructor.jl:46-82   (topology is *read*, never rebuilt)
 *   dojo_set_options   <- SolverOptions{T}                     src/solver/options.jl:16-26
 *   dojo_step          <- step!(mechanism, z, u; opts)         src/simulation/step.jl:11-30
 *                         (= set_maximal_state! + set_input! + mehrotra! + update_state!)
 *                         mehrotra!(mechanism; opts)           src/solver/mehrotra.jl:9-73
 *   dojo_get_solution  <- get_solution(mechanism)              src/gradients/finite_difference.jl:1-18
 *                         (what the Julia shim writes back into body.state.vsol/ωsol,
 *                          joint.impulses[2], contact.impulses_dual[2]/impulses[2] so that
 *                          DojoEnvironments.get_state, ant_ars.jl:72-80, keeps working)
 *   dojo_gradients     <- get_maximal_gradients!(mechanism, z, u; opts) / get_maximal_gradients(mechanism)
 *                         src/gradients/state.jl:69-126
 *   dojo_rollout       <- simulate!(mechanism, steps, storage, control!)  src/simulation/simulate.jl:16-36
 *                         with the control callback replaced by pre-sampled inputs U[k]
 *   dojo_set_external_force <- set_external_force!(body; force, torque, vertex)  src/bodies/set.jl:110-115
 *   dojo_simulate      <- simulate!(...; record = true): the same rollout, recording save_to_storage! rows
 *                         src/simulation/storage.jl:50-67, momentum(mechanism, body) src/mechanics/momentum.jl:17-41
 *   dojo_observe       <- get_state(environment)  DojoEnvironments/src/environments.jl:100-102,
 *                         environments/ant_ars.jl:72-80, environments/quadruped_sampling.jl:67-72
 *   dojo_contact_gradients <- get_contact_gradients(mechanism) src/gradients/contact.jl:1-55
 *   dojo_rollout_data_gradients / dojo_set_contact_data <- get_contact_gradients src/gradients/contact.jl:1-55, chained as in
 *                         examples/system_identification/utilities.jl:42-90 (set_data!(mechanism.contacts, theta), utilities.jl:52)
 *   dojo_minimal_to_maximal / dojo_maximal_to_minimal / dojo_step_minimal / dojo_minimal_gradients
 *                      <- minimal_to_maximal, maximal_to_minimal  src/mechanism/state.jl:9-66,
 *                         step_minimal_coordinates!               src/simulation/step.jl:42-60,
 *                         get_minimal_gradients!                  src/gradients/state.jl:183-217
 *   dojo_destroy       <- (GC of the Mechanism)
 *
 * All matrices at the ABI are row-major with the environment (batch) index slowest:
 * z[B][13*Nb], u[B][nu], dz[B][12*Nb][12*Nb], du[B][12*Nb][nu] -- except the Jacobians the `_dev` variants leave on
 * the device, which are column-major per environment (dz[B][column][row]: Julia-native, and what the kernels write coalesced).  Scalars are fp64
 * (dtype 0) or fp32 (dtype 1) as chosen at dojo_create; topology/option structs are
 * always fp64 and are cast on upload.  All arithmetic is fp64 in both modes.  An fp32 buffer cannot hold a unit
 * quaternion: with dtype 1 the state a z stands for is (x, v, q/|q|, omega), the kernels normalize q on load (the
 * reference never renormalizes; its formulas mix rotation_matrix, which scales with |q|^2, and vector_rotate, which
 * does not, so a 1e-7 norm error would otherwise be amplified by stiff contacts).  Differentiable steps of a dtype-1 handle keep an
 * internal fp64 work buffer of 8 * 18 * lanes/2 bytes per environment group and gradient column batch (Ant: 129 KB per
 * environment) so that fp32 outputs carry fp32 rounding only.  No exception crosses the boundary: every entry
 * point returns DOJO_OK (0) or a negative error code; dojo_last_error() gives the text of the last
 * failure in the process (one mutex-guarded string) and dojo_handle_error(h) the last failure on that handle.
 *
 * Pointer arguments are *host* pointers for the plain entry points and *device*
 * pointers for the `_dev` variants (used by bench.py / torch so that inputs are
 * resident in HBM when the timed region starts).  The host-pointer entry points synchronize the DEVICE
 * (hipDeviceSynchronize), not a stream: they may follow `_dev` calls that ran on caller streams the handle does not
 * keep (a non-blocking caller stream is not ordered with the null stream), and they move their data over PCIe anyway;
 * latency-sensitive callers stay on the `_dev` variants, which never synchronize.
 */
#ifndef DOJO_HIP_H
#define DOJO_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DOJO_OK                 0
#define DOJO_ERR_INVALID       -1   /* bad argument / malformed topology            */
#define DOJO_ERR_UNSUPPORTED   -2   /* e.g. kinematic loop, >1 parent joint per body */
#define DOJO_ERR_DEVICE        -3   /* HIP runtime error (text in dojo_last_error)   */
#define DOJO_ERR_NO_DEVICE     -4   /* no gfx950 device visible                      */

/* per-environment solver status, mirrors mehrotra!'s :success / :failed and the
 * "Excessive angular velocity" error() of src/solver/line_search.jl:18-20 */
#define DOJO_STATUS_SUCCESS      0
#define DOJO_STATUS_FAILED       1
#define DOJO_STATUS_EXCESSIVE_W  2

#define DOJO_DTYPE_F64 0
#define DOJO_DTYPE_F32 1

/* Body{T}: src/bodies/constructor.jl:14-27 (mass, inertia only; state is per-env) */
typedef struct DojoBody {
    double mass;
    double inertia[9];            /* row-major 3x3, body (COM) frame */
} DojoBody;

/*
 * JointConstraint{T,N,Nc,TJ,RJ} = Translational half + Rotational half
 * (src/joints/constraints.jl:17-86, translational/constructor.jl:18-67,
 *  rotational/constructor.jl:18-63).  Masks are exported from the live Julia object
 * (they come from an SVD, src/joints/orthogonal.jl:1-12) as
 *   cmask = constraint_mask(joint)  (nl   x 3, rows beyond nl   are ignored)
 *   amask = nullspace_mask(joint)   (3-nl x 3, rows beyond 3-nl are ignored)
 * (src/joints/joint.jl:56-64).
 */
typedef struct DojoJointHalf {
    int32_t nl;                   /* N-lambda: number of constrained directions, 0..3      */
    int32_t nlim;                 /* Nb/2: number of limited minimal coordinates (0..3-nl) */
    double  cmask[9];
    double  amask[9];
    double  spring;               /* joint.spring coefficient                              */
    double  damper;               /* joint.damper coefficient                              */
    double  spring_offset[3];     /* length 3-nl                                           */
    double  limit_lo[3];          /* joint_limits[1], length nlim                          */
    double  limit_hi[3];          /* joint_limits[2], length nlim                          */
} DojoJointHalf;

typedef struct DojoJoint {
    int32_t parent;               /* index into bodies[], -1 = origin (parent_id == 0)     */
    int32_t child;                /* index into bodies[]                                   */
    int32_t spring_on;            /* JointConstraint.spring flag                           */
    int32_t damper_on;            /* JointConstraint.damper flag                           */
    double  vertex_parent[3];     /* translational.vertices[1]                             */
    double  vertex_child[3];      /* translational.vertices[2]                             */
    double  orientation_offset[4];/* rotational.orientation_offset (s, v1, v2, v3)         */
    DojoJointHalf tra;
    DojoJointHalf rot;
} DojoJoint;

/* ContactConstraint{T,8,1,NonlinearContact,4} with SphereHalfSpaceCollision, child = origin
 * (src/contacts/nonlinear.jl:12-48, src/contacts/collisions/sphere_halfspace.jl:11-22) */
typedef struct DojoContact {
    int32_t body;                 /* parent_id as index into bodies[]                      */
    int32_t model;                /* 0: NonlinearContact (src/contacts/nonlinear.jl), 1: ImpactContact (src/contacts/impact.jl),
                                     2: LinearContact (src/contacts/linear.jl: friction pyramid, cone variables [gamma psi beta1..4]);
                                     1 and 2 forward only: the reference has no data Jacobians for them (src/gradients/data.jl:152-192);
                                     one model per mechanism; 2: <= 16 bodies, <= 4 contacts per body                        */
    double  friction_coefficient;
    double  normal[3];            /* collision.contact_normal (1x3)                        */
    double  tangent[6];           /* collision.contact_tangent (2x3, row-major)            */
    double  origin[3];            /* collision.contact_origin                              */
    double  radius;               /* collision.contact_radius                              */
    double  offset[3];            /* collision.contact_offset                              */
    /* body-body contact (src/contacts/collisions/sphere_sphere.jl:11-16; forward only; any of the three contact models): `body` is the contact's parent_id, its sphere is
     * (origin, radius); the child sphere sits on child_body, which must be a body whose joint hangs on `body` (the contact is an edge of
     * the tree next to that joint; the reference's test mechanism has no joint there at all: give the child a Floating joint to `body`).
     * normal / tangent / offset are unused. */
    int32_t collision;            /* 0: SphereHalfSpaceCollision (child = origin), 1: SphereSphereCollision */
    int32_t child_body;           /* collision 1: child_id as index into bodies[]; else ignored */
    double  child_origin[3];      /* collision 1: collision.origin_child                    */
    double  child_radius;         /* collision 1: collision.radius_child                    */
} DojoContact;

typedef struct DojoTopology {
    int32_t n_bodies, n_joints, n_contacts, reserved;
    double  timestep;
    double  input_scaling;
    double  gravity[3];
    const DojoBody*    bodies;    /* mechanism.bodies   order (defines the z layout)       */
    const DojoJoint*   joints;    /* mechanism.joints   order (defines the u layout)       */
    const DojoContact* contacts;  /* mechanism.contacts order                              */
} DojoTopology;

/* SolverOptions{T}: src/solver/options.jl:16-26 (ls_scale is unused by the reference,
 * halving is hard-coded in src/solver/line_search.jl:143; verbose has no device meaning) */
typedef struct DojoSolverOptions {
    double  rtol;                 /* 1e-6 */
    double  btol;                 /* 1e-4 */
    double  undercut;             /* Inf  */
    double  no_progress_undercut; /* 10   */
    int32_t max_iter;             /* 50   */
    int32_t max_ls;               /* 10   */
    int32_t no_progress_max;      /* 3    */
    int32_t reserved;
} DojoSolverOptions;

typedef struct DojoSim* DojoHandle;

/* dimensions derived from the topology (same formulas as the reference) */
typedef struct DojoDims {
    int32_t n_bodies, n_joints, n_contacts;
    int32_t nz;                   /* 13*Nb  maximal state                                  */
    int32_t nx;                   /* 12*Nb  attitude-reduced state (gradient rows/cols)    */
    int32_t nu;                   /* sum over joints of (3-nl_tra)+(3-nl_rot)              */
    int32_t n_joint_impulses;     /* sum over joints of N_j = sum_halves nl + 4*nlim       */
    int32_t n_solution;           /* n = n_joint_impulses + 6*Nb + 8*Nc                    */
    int32_t lanes_per_env;        /* S: wavefront lanes cooperating on one environment     */
} DojoDims;

/* gradient flavour, SURVEY.md §8a note Q2 */
#define DOJO_GRAD_REFERENCE  0    /* literal get_maximal_gradients! (data blocks on the post-update_state! state) */
#define DOJO_GRAD_CONSISTENT 1    /* data blocks on the pre-update state (what test/data.jl checks)               */

int  dojo_device_count(void);
const char* dojo_last_error(void);
/* text of the last failure of a call on THIS handle ("" if none): per-handle, safe with several handles on several threads */
const char* dojo_handle_error(DojoHandle h);

int  dojo_create(const DojoTopology* topo, int32_t batch, int32_t dtype, int32_t device, DojoHandle* out);
void dojo_destroy(DojoHandle h);
int  dojo_get_dims(DojoHandle h, DojoDims* dims);
int  dojo_set_options(DojoHandle h, const DojoSolverOptions* opts);
int  dojo_set_gradient_mode(DojoHandle h, int32_t mode);
/* Accuracy of the device's linear solves.  The reference's block LDU (GraphBasedSystems, call sites
 * src/solver/mehrotra.jl:36-37,49 and the dense `\` of src/gradients/state.jl:99) is an exact direct method; the device
 * eliminates contacts and limits first, which in fp64 costs log10(gamma/s) digits of the body blocks.  Environments whose
 * cones reach max gamma/s > stiffness therefore get every Newton and IFT solve refined against the un-eliminated KKT system
 * (DESIGN.md section 4.5).  INFINITY = never, 0 = always, negative = the default policy: DOJO_DEFAULT_REFINE_STIFFNESS when the
 * solver tolerances are rtol <= 1e-7 or btol <= 1e-6, never at the reference's default tolerances. */
#define DOJO_DEFAULT_REFINE_STIFFNESS 1.0e4
int  dojo_set_refinement(DojoHandle h, double stiffness);

/* step!: z [B,13Nb], u [B,nu] (NULL = zeros) -> z_next [B,13Nb] = the mechanism's internal
 * state after update_state! (x3,v25,q3,w25; SURVEY §8a note Q1), status [B], iters [B]
 * (status / iters may be NULL).  with_gradient != 0 additionally leaves the IFT Jacobians
 * of this step in the handle for dojo_gradients(). */
int  dojo_step(DojoHandle h, const void* z, const void* u, void* z_next,
               int32_t* status, int32_t* iters, int32_t with_gradient);

/* mehrotra!(mechanism; opts)  src/solver/mehrotra.jl:9 -- the seam a single-`Mechanism` drop-in overrides.
 * When mehrotra! runs, set_input! / input_impulse! (src/mechanism/set.jl:40-53, src/joints/translational/input.jl:5-27,
 * src/joints/rotational/input.jl:5-17) have already turned the controls into body impulses and cleared the joints' inputs:
 * jf [B, 6Nb] = per body [state.JF2 (world frame, 3); state.Jtau2 (body frame, 3)], exactly the vector the body residual
 * subtracts (src/integrators/constraint.jl:20-21).  Equivalent to dojo_step(z, u) for the u that produced jf; any
 * external force set with dojo_set_external_force stays in effect.  z, z_next, status, iters as for dojo_step. */
int  dojo_step_impulses(DojoHandle h, const void* z, const void* jf, void* z_next, int32_t* status, int32_t* iters);

/* The vector the reference's step! literally returns (src/simulation/step.jl:28: get_next_state AFTER update_state!, i.e. the
 * internal next state advanced once more with its own velocities -- SURVEY.md section 8a Q1).  dojo_step / dojo_rollout return
 * the internal state (x3, v25, q3, w25), which is what the next step and DojoEnvironments' get_state consume; this maps it to
 * the literal return value: z_out = (x3 + dt v25, v25, q3 (x) xi(w25), w25) per body (src/mechanism/get.jl:126-134). */
int  dojo_next_state(DojoHandle h, const void* z, void* z_out);
int  dojo_next_state_dev(DojoHandle h, const void* z, void* z_out, void* stream);

/* solution of the last step in get_solution order per env:
 * vel [B,6Nb] (v25,w25 per body), joint_imp [B,n_joint_impulses], contact_sg [B,8Nc] ([s(4);gamma(4)] per contact; an
 * ImpactContact uses the first of each four; LinearContact mechanisms: [B,12Nc], [s(6);gamma(6)]).
 * Any pointer may be NULL. */
int  dojo_get_solution(DojoHandle h, void* vel, void* joint_imp, void* contact_sg);
/* mechanism.mu (the central-path parameter kappa of the docs, src/solver/mehrotra.jl:45) per environment when the solve of
 * the last step returned, fp64 [B]: a mehrotra! drop-in writes it back and calls set_entries! so that mechanism.system
 * holds the final un-factored Jacobian and residual like the reference leaves it (src/solver/mehrotra.jl:69). */
int  dojo_get_mu(DojoHandle h, double* mu);
/* Diagnostics of the LAST LINEARIZATION PERFORMED in every environment's last step (quad mappings; without the refining kernels a step skips
 * the set_entries! after its converging iteration, so this is the linearization one iterate before the solution), fp64 [B, 2]: [0] max gamma/s over
 * its cones (what dojo_set_refinement's threshold is compared with), [1] the largest multiplier of the device's un-pivoted
 * Gauss-Jordan eliminations.  The first call switches the recording on (diag may be NULL), later calls read the last step.
 * [0] is 0 while no refinement threshold is in force (reference-default options and no dojo_set_refinement: the kernels then
 * skip the stiffness arithmetic); [1] is 0 unless the library was built with -DDJ_TRACK_GROWTH=1 (a diagnostics build). */
int  dojo_get_diagnostics(DojoHandle h, double* diag);
/* Which kernel build steps this handle (read-only; no GPU work): out = [family, MAXC, waves].  family: 0 plain, 1 translational springs / dampers
 * (tsd), 2 general (limits on several coordinates, loops), 3 LinearContact, 4 body-body contacts.  MAXC: the build's bound on contacts per body.
 * waves: wavefronts per workgroup of the quad mapping (1, 2), 0 = lane mapping.  DOJO_ERR_UNSUPPORTED when no build serves the mechanism. */
int  dojo_get_kernel_build(DojoHandle h, int32_t out[3]);

/* IFT Jacobians of the last dojo_step(..., with_gradient=1):
 * dz [B,12Nb,12Nb] = jacobian_state, du [B,12Nb,nu] = jacobian_control, row-major per environment
 * (transposed on the device from the kernels' column-major layout) */
int  dojo_gradients(DojoHandle h, void* dz, void* du);

/* simulate! with pre-sampled controls: z0 [B,13Nb], U [H,B,nu] (NULL = zeros) ->
 * Z [H,B,13Nb] (state after each step; NULL = keep only the final state, readable with
 * dojo_get_state), status [H,B] (may be NULL) */
int  dojo_rollout(DojoHandle h, const void* z0, const void* U, int32_t H, void* Z, int32_t* status);
int  dojo_get_state(DojoHandle h, void* z);

/* device-pointer variants: all pointers are device memory on the handle's GPU, work is
 * enqueued on `stream` (a hipStream_t passed as void*, NULL = the null stream) and NOT
 * synchronized; outputs are valid after the stream is synchronized. */
int  dojo_step_dev(DojoHandle h, const void* z, const void* u, void* z_next,
                   int32_t* status, int32_t* iters, void* dz, void* du, void* stream);
/* Environment groups.  Environments are independent, so dojo_step_dev steps a batch of >= 512 environments as up to 16
 * groups on internal HIP streams (of >= 256 environments each; an asynchronous handle, below, of a mechanism with one
 * wavefront per workgroup: of >= 64 workgroups, so that batches of 128 .. 2048 Ants are split further): a group that holds an environment running into max_iter (~5x the mean step time for
 * its wavefront) delays only itself.  By default the call forks from and joins into `stream`, i.e. it behaves like one
 * launch on `stream` (such a joined handle steps a batch of more workgroups than the GPU holds at once as TWO groups: each launch has the whole GPU for its
 * rounds of workgroups, the first group's IFT kernel runs under the tail of the second's step kernel; see dojo_set_dispatch_order).  dojo_set_async(h, 1) drops the join: consecutive dojo_step_dev calls then chain per group (group g
 * of call k+1 runs behind group g of call k and behind what `stream` held at call time), and dojo_join(h, stream)
 * -- or any host-pointer entry point -- orders `stream` behind everything in flight.  The caller must not touch the
 * outputs, nor overwrite the inputs, of un-joined calls.  dojo_set_groups(h, n): n groups, at most 16 (n <= 0: automatic; 1: a
 * single launch on the caller's stream).  ROCm runs at most GPU_MAX_HW_QUEUES (default 4) streams concurrently: set it
 * to >= groups + 1 before the HIP runtime starts.  (No counterpart in the reference, which is single-threaded.)
 * dojo_set_async(h, 2): asynchronous AND pipelined -- the IFT kernel of a group's step k runs on a second internal stream of the group, behind
 * its step kernel and NEXT TO the step kernel of step k + 1 (both depend on step k alone; two step -> IFT hand-off records in turn), so that the
 * SIMDs a draining step kernel leaves idle find work.  Same contract (inputs and outputs of un-joined calls stay untouched -- here the IFT of
 * step k still reads z, u of step k while step k + 1 runs: do not hand step k's z in as z_next of step k + 1); dz / du of consecutive calls
 * are written in call order.  Plain solves only (with refinement in force the groups run as under 1); 2 x groups + 1 hardware queues.
 * Where it pays: batches that leave SIMDs idle (Atlas at B = 256 in two groups: 155 k -> 240 k env-steps/s, B = 512: 260 k -> 300 k,
 * profiles/r06_g_pipeline.txt); at batches that fill the GPU the plain groups are as fast or faster (Ant B = 1024 .. 4096: -3 .. -5 %). */
int  dojo_set_async(DojoHandle h, int32_t on);
int  dojo_set_groups(DojoHandle h, int32_t n);
/* Iteration cap of the step kernel (no counterpart in the reference; the algorithm is unchanged decision for decision).  `mehrotra!` (src/solver/
 * mehrotra.jl:9-73) is a serial chain of up to max_iter Newton iterations per environment, and an iteration whose line search is exhausted
 * evaluates the residual up to max_ls times in a row (src/solver/line_search.jl:1-34).  With a cap, a step that is joined into the caller's
 * stream (dojo_step, dojo_step_dev of a handle that is not asynchronous) runs in phases: the step kernel hands every solve that is unfinished
 * after `cap` iterations to a continuation kernel, in which several wavefronts hold the same environment and evaluate the line-search trials
 * alpha, alpha/2, alpha/4, ... side by side before replaying line_search!'s accept / halve decisions over the results; the IFT kernel of the
 * finished environments runs next to it.  Results: bit for bit those of the uncapped loop under the SIMT emulator; on the GPU the continuation
 * kernel is a second instantiation of the lane program (other fused multiply-add contractions), so a continued solve differs in its last bits.
 * Measured on MI355X: a stalled iteration takes 0.087 instead of 0.110 ms; joined Ant steps gain 10 % at B = 512, 4 % at
 * B = 2048 and lose 3 % at B = 4096 (the IFT can no longer start behind its own group's step kernel) -- hence OFF by default.
 * cap > 0: in force for joined steps of the single-wavefront quad mapping (<= 16 bodies) without refinement; 0 or < 0: off (the default; the
 * environment variable DOJO_ITER_CAP=<cap> changes the default, not an explicit setting).  Asynchronous handles and rollouts never cap. */
#define DOJO_DEFAULT_ITERATION_CAP 0
int  dojo_set_iteration_cap(DojoHandle h, int32_t cap);
/* Order in which the step kernel's workgroups are handed to the GPU (no counterpart in the reference: mehrotra!, src/solver/mehrotra.jl:9-73, runs
 * one mechanism).  A launch ends with its last wavefront, and the Newton loops of a batch take 5 ... max_iter iterations: a 50-iteration solve that
 * starts in the launch's last round of workgroups IS that wavefront.  A solve that was long in one step is long in the next (the same contacts are
 * closing), so the library sorts the workgroups of a launch by the iteration counts of the previous step, longest first (a one-workgroup counting
 * sort behind the step's kernels; the step kernel reads its workgroup index through the permutation).
 * mode 0: batch order.  1 (default): sorted where it can matter -- steps joined into the caller's stream (or stepped as a single group) whose batch has
 * more workgroups than the GPU holds at once (asynchronous handles of several groups hide the tail behind the other groups' kernels).  2: always.  Results do not depend on the order: every
 * environment is computed by the same program wherever it runs.  Measurements: DESIGN.md section 6. */
int  dojo_set_dispatch_order(DojoHandle h, int32_t mode);
int  dojo_join(DojoHandle h, void* stream);

/* Multi-GPU (nothing to cite in the reference, which has no multi-device code).  Environments are
 * independent: one process per GPU, each with ONE handle for its contiguous slice of the batch (rank r of W owns the r-th
 * slice), topology and options replicated, no exchange inside the solver.  The only collective is an all-gather of per-rank
 * outputs over RCCL / xGMI, once per rollout chunk:
 *   dojo_comm_unique_id(id)            rank 0: 128 opaque bytes, which the host passes to the other ranks (Julia Distributed,
 *                                      MPI, torch.distributed ...)
 *   dojo_comm_init(h, rank, world, id) every rank: joins the handle's device into the communicator
 *   dojo_allgather_dev(h, send, recv, count, as_int32, stream)
 *                                      recv[world][count] <- send[count] of every rank, in rank order (= batch order);
 *                                      elements are scalars of the handle's dtype, or int32 (status) with as_int32 != 0;
 *                                      ordered on `stream` behind everything the handle has in flight
 * RCCL is loaded on first use (dlopen), single-GPU callers never touch it. */
int  dojo_comm_unique_id(void* id128);
int  dojo_comm_init(DojoHandle h, int32_t rank, int32_t world, const void* id128);
int  dojo_allgather_dev(DojoHandle h, const void* send, void* recv, int64_t count, int32_t as_int32, void* stream);
int  dojo_comm_info(DojoHandle h, int32_t* rank, int32_t* world);
int  dojo_rollout_dev(DojoHandle h, const void* z0, const void* U, int32_t H, void* Z,
                      int32_t* status, void* stream);

/* set_external_force!(body; force, torque, vertex)  src/bodies/set.jl:110-115, read by the body residual
 * src/integrators/constraint.jl:15-18 (state.Fext, state.τext; a3 of SURVEY.md §8a).  fext [B, 6Nb]: per body the force
 * in the world frame and the torque in the body frame, i.e. the two state fields after the reference's
 * `vertex` arithmetic.  The forces stay in effect for every following step of the handle (step!, which never clears
 * them; a rollout applies them at every step, as a controller that sets them at every step) until they are replaced
 * or removed with NULL.  The host variant copies; the device variant keeps the caller's pointer. */
int  dojo_set_external_force(DojoHandle h, const void* fext);
int  dojo_set_external_force_dev(DojoHandle h, const void* fext);

/* simulate!(mechanism, 1:H, storage, control!; record = true)  src/simulation/simulate.jl:16-37  (SURVEY.md §8f-2):
 * dojo_rollout plus the Storage of the trajectory, written by the step kernel itself.  storage [H, B, Nb, 25], one
 * save_to_storage! row (src/simulation/storage.jl:50-67) per solved step and body, taken BEFORE update_state! as
 * simulate! does:  x2(3) q2(4) v15(3) omega15(3) | px(3) pq(3) (momentum(mechanism, body), world frame,
 * src/mechanics/momentum.jl:17-41) | vl(3) = px / m, omegal(3) = J \ (pq in the body frame).
 * Z and status as for dojo_rollout (both may be NULL). */
int  dojo_simulate(DojoHandle h, const void* z0, const void* U, int32_t H, void* Z, void* storage, int32_t* status);
int  dojo_simulate_dev(DojoHandle h, const void* z0, const void* U, int32_t H, void* Z, void* storage,
                       int32_t* status, void* stream);

/* Reverse-mode rollouts (no counterpart in the reference, which differentiates one step at a time: get_maximal_gradients!,
 * src/gradients/state.jl:69-126): the gradient of a trajectory loss w.r.t. the control sequence and the initial state, from the IFT
 * Jacobians of every step, which stay on the device.
 *
 * dojo_rollout_record_dev = dojo_rollout_dev plus the record: DZ [H][B][nx][nx] and DU [H][B][nu][nx] in the device layout of
 * dojo_step_dev (column-major per environment: DZ[k][b][c][r] = d x_{k+1}[r] / d x_k[c]; DU is ignored when nu = 0).  Z is required
 * (the reverse sweep may need it); status may be NULL.  Same environment groups and stream choreography as dojo_rollout_dev: joined into
 * `stream` at the end, never pipelined.  The Jacobians are those of the handle's gradient mode (dojo_set_gradient_mode):
 * DOJO_GRAD_CONSISTENT is the one whose chain is the derivative of the rollout (rows of step k and columns of step k + 1 then live in
 * the same tangent coordinates [x; v; phi; omega] per body); DOJO_GRAD_REFERENCE chains the reference's literal blocks.  ImpactContact,
 * LinearContact and body-body contact mechanisms: DOJO_ERR_UNSUPPORTED, nothing launched.
 * Memory of the record: H * B * nx * (nx + nu) * w bytes (w = 8 or 4) -- Ant (nx 156, nu 14), fp32, B = 4096, H = 20: 8.7 GB.
 *
 * dojo_rollout_adjoint_dev: ONE kernel launch on `stream`, no synchronization; plain device buffers in the handle's dtype, from
 * dojo_rollout_record_dev or from the caller's own dojo_step_dev loop (closed-loop policies).  With g_k the cotangent of the loss w.r.t.
 * the state after step k (k = 0 .. H-1), per environment b:
 *     lambda <- g_{H-1}
 *     for k = H-1 .. 0:   if status && status[k][b] != 0:  gU[k][b] <- 0;                  lambda <- 0
 *                         else:                            gU[k][b] <- DU_k[b]^T lambda;   lambda <- DZ_k[b]^T lambda
 *                         if k > 0: lambda <- lambda + g_{k-1}
 *     gz[b] <- lambda                                      (tangent coordinates, [B][nx])
 * Nothing flows through a failed step, by select: its Jacobians need not be finite and are not read.
 * cot_space 0: G [H][B][nx] is given in the tangent coordinates of dz; Z may be NULL.  cot_space 1: G [H][B][13Nb] is given in state
 * coordinates and Z [H][B][13Nb] is required: per body g_x, g_v, g_omega are copied and g_phi = vector part of conj(q) (x) g_q (the
 * transpose of dq/dphi = LV^T mat(q); fp32 handles use q / |q|, as the kernels do on load).
 * status, gU [H][B][nu] and gz may each be NULL; gU is ignored when nu = 0.  Every product and sum is fp64, lambda stays fp64 between the
 * steps, outputs are rounded once.  No atomics and a fixed summation order: results are bit-identical from run to run and do not depend
 * on the batch size or on an environment's position in the batch.  DOJO_ERR_INVALID (text on the handle): H < 1, NULL DZ or G,
 * cot_space = 1 without Z, gU without DU (nu > 0), DZ or DU not 16-byte aligned (the kernel reads them in 16-byte pieces; every
 * environment's block and column then is, since nx = 12 Nb -- hipMalloc and torch allocations are aligned, an offset into one need not be).
 *
 * dojo_rollout_gradients (host pointers): uploads z0, U (NULL = zeros), G; allocates the record on the device, records, runs the reverse
 * sweep, downloads Z [H][B][13Nb], status [H][B], gU [H][B][nu], gz [B][nx] (each may be NULL).  The Jacobians never cross PCIe.  A record
 * that does not fit into the free device memory: DOJO_ERR_INVALID with the byte count in the text, before any launch. */
int  dojo_rollout_record_dev(DojoHandle h, const void* z0, const void* U, int32_t H, void* Z, int32_t* status,
                             void* DZ, void* DU, void* stream);
int  dojo_rollout_adjoint_dev(DojoHandle h, int32_t H, const void* DZ, const void* DU, const void* G, int32_t cot_space,
                              const void* Z, const int32_t* status, void* gU, void* gz, void* stream);
int  dojo_rollout_gradients(DojoHandle h, const void* z0, const void* U, int32_t H, const void* G, int32_t cot_space,
                            void* Z, int32_t* status, void* gU, void* gz);

/* Contact-parameter gradients through rollouts (system identification): get_contact_gradients, src/gradients/contact.jl:1-55, chained as in
 * examples/system_identification/utilities.jl:42-90 -- here in reverse mode, on the device (csrc/dojo_data_adjoint.hpp).
 *
 * theta is the contact data of get_contact_gradients: 5 values per contact, [friction_coefficient, contact_radius, contact_origin(3)], in
 * mechanism.contacts order -- [Nc][5], n_theta = 5 Nc.  It is mechanism data, SHARED by all environments of a handle.  (One theta per
 * environment would put the contact table on the batch axis of the step kernel: not supported.)
 *
 * dojo_set_contact_data: set_data!(mechanism.contacts, theta) on a live handle.  Joins the handle's environment groups, waits for the work
 * in flight, replaces friction coefficient, radius and origin of every contact and uploads the contact table again; the handle then steps
 * bit-identically to one created with theta.  The solution of an earlier differentiable step no longer belongs to the handle's data:
 * dojo_contact_gradients fails until the next dojo_step(..., with_gradient = 1).  theta is a HOST pointer (fp64, whatever the handle's
 * dtype).  DOJO_ERR_INVALID: a negative or non-finite friction coefficient or radius, a non-finite origin.  DOJO_ERR_UNSUPPORTED: a
 * non-zero friction coefficient on an ImpactContact (it has none: pass 0).  Nothing is changed when a value is refused.
 * dojo_get_contact_data: the handle's current theta.  With Nc = 0 both return DOJO_OK and touch nothing.
 *
 * dojo_rollout_data_record_dev = dojo_rollout_record_dev plus DC [H][B][5Nc][nx]: for every step the contact-data columns in the layout
 * dojo_contact_gradients_dev writes (column-major per environment, DC[k][b][c][r] = d x_{k+1}[r] / d theta[c]: a column holds nx
 * contiguous rows).  On a failed step DC[k][b], like DZ[k][b], holds nothing of use.  Refused like dojo_contact_gradients_dev, before
 * anything is allocated or launched: body-body contacts, ImpactContact / LinearContact, more than 64 contacts, mechanisms outside the
 * quad mapping (> 32 bodies).  DC == NULL: the call IS dojo_rollout_record_dev.
 * Memory of the record: H * B * nx * (nx + nu + 5 Nc) * w bytes -- Ant (nx 156, nu 14, Nc 4), fp32, B = 4096, H = 20: 9.7 GB.
 *
 * dojo_rollout_data_adjoint_dev: ONE sweep launch on `stream` (plus a small reduction when gtheta is wanted), no synchronization.  With
 * g_k as in dojo_rollout_adjoint_dev (G, cot_space, Z, status have the same meaning), per environment b:
 *     lambda <- g_{H-1};  a <- 0
 *     for k = H-1 .. 0:   if status && status[k][b] != 0:  lambda <- 0                           (DZ_k, DC_k are not read)
 *                         else:                            a <- a + DC_k[b]^T lambda;   lambda <- DZ_k[b]^T lambda
 *                         if k > 0: lambda <- lambda + g_{k-1}
 *     gtheta_env[b] <- a   [B][5Nc];    gz[b] <- lambda   [B][nx], tangent coordinates;    gtheta <- sum_b a_b   [5Nc]
 * Each output may be NULL, not all three.  Every product and sum is fp64, lambda and a stay fp64 between the steps, outputs are rounded
 * once (gtheta after the sum over the batch).  No atomics, fixed summation orders: all outputs are bit-identical from run to run;
 * gtheta_env and gz do not depend on the batch size or on an environment's position in the batch (the sum gtheta does: its order is
 * fixed by B).  The gradient w.r.t. the controls is dojo_rollout_adjoint_dev's, over the same record.
 * DOJO_ERR_INVALID (text on the handle, nothing launched): H < 1; NULL DZ or G; NULL DC with Nc > 0; all three outputs NULL;
 * cot_space = 1 without Z; DZ or DC not 16-byte aligned.  Nc = 0: gz is computed, gtheta_env and gtheta are not touched.
 *
 * dojo_rollout_data_gradients (host pointers): uploads z0, U (NULL = zeros), G; allocates the record on the device, records, runs the
 * sweep above -- and dojo_rollout_adjoint_dev over the same record when gU is not NULL --, downloads Z, status, gtheta [5Nc],
 * gtheta_env [B][5Nc], gU [H][B][nu], gz [B][nx] (each may be NULL).  A record that does not fit into the free device memory:
 * DOJO_ERR_INVALID with the byte count in the text, before any launch. */
int  dojo_set_contact_data(DojoHandle h, const double* theta /* [Nc][5] */);
int  dojo_get_contact_data(DojoHandle h, double* theta /* [Nc][5] */);
int  dojo_rollout_data_record_dev(DojoHandle h, const void* z0, const void* U, int32_t H, void* Z, int32_t* status,
                                  void* DZ, void* DU, void* DC /* [H][B][5Nc][nx] */, void* stream);
int  dojo_rollout_data_adjoint_dev(DojoHandle h, int32_t H, const void* DZ, const void* DC, const void* G, int32_t cot_space,
                                   const void* Z, const int32_t* status,
                                   void* gtheta_env /* [B][5Nc] or NULL */, void* gtheta /* [5Nc], summed over the batch, or NULL */,
                                   void* gz /* [B][nx] or NULL */, void* stream);
int  dojo_rollout_data_gradients(DojoHandle h, const void* z0, const void* U, int32_t H, const void* G, int32_t cot_space,
                                 void* Z, int32_t* status, void* gtheta, void* gtheta_env, void* gU, void* gz);

/* Forward-mode rollouts: T tangent directions swept over a record in ONE pass (csrc/dojo_tangent.hpp) -- the chain that the reference's system
 * identification runs on the host, step by step (examples/system_identification/utilities.jl:42-90): J v next to the J^T w of the entries above
 * (Gauss-Newton / Levenberg-Marquardt products J^T Q J v: two sweeps over one record; the sensitivities of a whole trajectory to a few parameters).
 *
 * dojo_rollout_tangent_dev: ONE launch for all H steps on `stream`, no synchronization.  DZ, DU, DC are plain device buffers in the handle's
 * dtype, as dojo_rollout_record_dev / dojo_rollout_data_record_dev (or the caller's own step loop) leave them.  Per environment b, tangent t:
 *     delta <- dz0[b][t]                                                        dz0 [B][T][nx], tangent coordinates [x; v; phi; omega] per body
 *     for k = 0 .. H-1:   if status && status[k][b] != 0:  delta <- 0           (DZ_k, DU_k, DC_k are not read: they may be NaN)
 *                         else:  delta <- DZ_k[b] delta + DU_k[b] dU[k][b][t] + DC_k[b] dtheta[t]      dU [H][B][T][nu], dtheta [T][5Nc] (shared by the batch)
 *                         dZ[k][b][t] <- delta
 * This is the transpose of the failure rule of the reverse sweeps: nothing flows through a failed step, the tangent of the state after it is 0,
 * later controls act again.  tan_space = 0: dZ [H][B][T][nx].  tan_space = 1: dZ [H][B][T][13Nb], the push-forward per body -- x, v, omega copied,
 * dq = q (x) (0, phi) with q from Z[k][b] (fp32 handles: q / |q|) --, the transpose of what cot_space = 1 does to a cotangent.
 * Each of dz0, dU, dtheta may be NULL (= zeros; the matching Jacobian array -- DU for dU, DC for dtheta -- is then not read and may be NULL); dU is
 * ignored when nu = 0, dtheta when Nc = 0.  Every product and sum is fp64, delta stays fp64 between the steps, outputs are rounded once.  No
 * atomics; the summation order is fixed by (nx, nu, 5Nc, dtype) alone: a tangent's result is bit-identical from run to run and does not depend on
 * B, on the environment's position in the batch, on T or on the tangent's position among the T.
 * DOJO_ERR_INVALID (text on the handle, nothing launched): H < 1 or T < 1; NULL DZ or dZ; dz0, dU and dtheta all NULL (after the two rules
 * above); dU without DU (nu > 0); dtheta without DC (Nc > 0); tan_space not 0 or 1; tan_space = 1 without Z; DZ, DU or DC not 16-byte aligned.
 * DOJO_ERR_UNSUPPORTED: a column of more than 256 16-byte pieces (one team of lanes sweeps a column: nx <= 512 in fp64, 1024 in fp32), or inputs
 * and partial sums of a step -- 32 (nx + nu + 5Nc + nteams nx) bytes, nteams = min(256 / pieces, 16) -- beyond 64 KB of LDS.  Atlas (nx 372) needs 40 KB.
 *
 * dojo_rollout_tangents (host pointers): uploads z0, U (NULL = zeros), dz0, dU, dtheta; allocates the record on the device -- DZ, DU only when dU
 * is given, DC only when dtheta is given --, runs the recording rollout and the sweep above, downloads Z [H][B][13Nb], status [H][B] (each may be
 * NULL) and dZ.  The Jacobians never cross PCIe.  Mechanisms the recording rollouts refuse are refused the same way.
 * Memory of the call, exactly what it allocates: the record, H B nx (nx + [nu] + [5Nc]) w bytes ([nu] with dU, [5Nc] with dtheta) -- Ant (nx 156,
 * nu 14, Nc 4), fp32, B = 4096, H = 20, all three: 9.7 GB --, the output H B T nout w (nout = nx or 13Nb), the states and status H B (13Nb w + 4),
 * the inputs that are given (z0 B 13Nb w, U H B nu w, dz0 B T nx w, dU H B T nu w, dtheta T 5Nc w), and the handle's workspaces on first use.  A
 * call that does not fit into the free device memory: DOJO_ERR_INVALID with the byte counts in the text, before any launch. */
int  dojo_rollout_tangent_dev(DojoHandle h, int32_t H, int32_t T, const void* DZ, const void* DU, const void* DC,
                              const void* dz0 /* [B][T][nx] or NULL */, const void* dU /* [H][B][T][nu] or NULL */, const void* dtheta /* [T][5Nc] or NULL */,
                              int32_t tan_space, const void* Z, const int32_t* status, void* dZ /* [H][B][T][nx or 13Nb] */, void* stream);
int  dojo_rollout_tangents(DojoHandle h, const void* z0, const void* U, int32_t H, int32_t T,
                           const void* dz0, const void* dU, const void* dtheta, int32_t tan_space, void* Z, int32_t* status, void* dZ);

/* Closed-loop rollouts: simulate!(mechanism, steps, storage, control!) (src/simulation/simulate.jl:16-37) with a controller that looks at the
 * state -- an affine feedback policy per environment, evaluated ON THE DEVICE between the steps (csrc/dojo_policy.hpp: observation, normalisation,
 * policy and control assembly in one launch), so that the call keeps the choreography of dojo_rollout_dev: environment groups chained on internal
 * streams, one join into `stream` at the end, no synchronization.  u = -K x (examples/control/cartpole_lqr.jl), the linear policy on normalised
 * observations of examples/learning/ant_ars.jl:78-115 (per_env = 1: one perturbed policy per environment) and PD around a reference (U_ff) are
 * all of this form:
 *
 *     u_k = U_ff[k] + E (bias + W ((o_k - mean) .* scale)),      o_k = get_state of the state step k starts from
 *
 * Per environment b and step k = 0 .. H-1, with z_0 = z0 and z_k = Z[k-1]:
 *   1. o_k = [maximal_to_minimal(z_k) (2 nu); c_k (Nc, only with contact_forces)], c_k = the normal impulse of every contact of step k - 1 clamped
 *      to [-1, 1] -- exactly dojo_observe_dev's vector; c_0 by contact_init.  o_k is rounded once to the handle dtype and written to OBS[k][b];
 *      THE POLICY CONSUMES THE ROUNDED VALUE: what is recorded is what it saw, and U_out can be recomputed from OBS alone.
 *   2. fp64: ohat_j = (o_j - mean_j) scale_j;  a_i = bias_i + sum_j W[i][j] ohat_j, in a summation order that depends on nobs alone.
 *   3. u = U_ff[k][b] (or zeros); u[act_off + i] += a_i; rounded once to the handle dtype, written to U_out[k][b]; step k reads exactly that buffer.
 *   4. step k, through the path of dojo_rollout_dev (external forces set on the handle stay in effect): Z[k], status[k].
 * After the last step OBS[H] = the observation of the final state (a reward r(o_k, u_k, o_{k+1}) needs it).
 * OBS [H+1][B][nobs], U_out [H][B][nu], Z [H][B][13Nb], status [H][B]: each may be NULL (with Z NULL the final state stays readable with
 * dojo_get_state).  Results are bit-identical from run to run and do not depend on the number of environment groups, on an environment's position
 * in the batch, or on per_env = 0 against the same W given B times.
 * The struct is host memory, read during the call; its members are device pointers (dojo_rollout_policy_dev) or host pointers (dojo_rollout_policy).
 * Refused before anything is launched, text on the handle -- DOJO_ERR_INVALID: NULL handle, z0, policy or W; H < 1; nu = 0; na < 1, act_off < 0 or
 * act_off + na > nu; contact_init = 1 on a handle without a solution.  DOJO_ERR_UNSUPPORTED: a mechanism with a kinematic loop, contact_forces with
 * LinearContact (both as dojo_observe_dev); more than 2048 observations.
 * Not part of it: contact observations in reverse mode (below), activations other than the tanh of the network policy (DojoMlpPolicy below), output
 * squashing, rewards / termination, running normaliser statistics, control clamping, re-projection to minimal coordinates between the steps (DojoEnvironments' step! does that; simulate! does not). */
typedef struct DojoPolicy {
    const void* W;        /* [Bw][na][nobs] row-major, handle dtype, device memory; required            */
    const void* bias;     /* [Bw][na] or NULL (zeros)                                                   */
    const void* mean;     /* [nobs] or NULL (zeros): shared by all environments                         */
    const void* scale;    /* [nobs] or NULL (ones)                                                      */
    const void* U_ff;     /* [H][B][nu] or NULL (zeros): feed-forward / exploration / PD reference term */
    int32_t per_env;      /* 1: Bw = B (one policy per environment, ARS directions); 0: Bw = 1 (shared) */
    int32_t act_off, na;  /* the policy drives inputs act_off .. act_off + na - 1 (E above)             */
    int32_t contact_forces;/* nobs = 2 nu + (contact_forces ? Nc : 0), as dojo_observe_dev              */
    int32_t contact_init; /* contact entries of o_0: 0 = the neutral 1.0 (a fresh ContactConstraint, what
                             BatchedEnvironment.get_state returns before the first step), 1 = the handle's last solution */
    int32_t reserved;
} DojoPolicy;
int  dojo_rollout_policy_dev(DojoHandle h, const void* z0, const DojoPolicy* policy, int32_t H,
                             void* Z, void* OBS, void* U_out, int32_t* status, void* stream);
int  dojo_rollout_policy(DojoHandle h, const void* z0, const DojoPolicy* policy, int32_t H,
                         void* Z, void* OBS, void* U_out, int32_t* status);

/* Reverse mode through closed-loop rollouts: the gradient of a trajectory loss w.r.t. the POLICY (W, bias), the feed-forward term and the initial
 * state -- what replaces the random search of examples/learning/ant_ars.jl with first-order optimisation.  No counterpart in the reference, which
 * differentiates one step at a time (src/gradients/state.jl:69-126).  csrc/dojo_policy_adjoint.hpp has the kernels.
 *
 * Per environment: z_0 = z0, z_k = Z[k-1]; o_k = the minimal-coordinate observation of z_k; ohat_k = (o_k - mean) .* scale, formed in fp64 from the
 * RECORDED, rounded OBS[k] exactly as the forward kernel forms it; u_k = U_ff[k] + E (bias + W ohat_k); M_k = d o_k / d z_k [2nu x nx] in the tangent
 * coordinates [x; v; phi; omega] per body (dq = q (x) (0, phi): the convention of dz and of cot_space = 1), evaluated at z_k itself.  With the
 * cotangents g_k (w.r.t. the state after step k), GU_k (w.r.t. U_out[k]) and GO_k (w.r.t. OBS[k], k = 0 .. H):
 *     lambda <- g_{H-1} + M_H^T GO_H;   gW <- 0;   gbias <- 0
 *     for k = H-1 .. 0:   if status && status[k][b] != 0:  lambda <- 0          (by select: DZ_k, DU_k need not be finite and are not read)
 *                         gu     = DU_k^T lambda + GU_k                          -> gU[k]   (gradient w.r.t. U_ff[k]; all nu entries)
 *                         a      = gu[act_off .. act_off + na - 1]
 *                         gbias += a;   gW += a ohat_k^T
 *                         go     = scale .* (W^T a) + GO_k
 *                         lambda = DZ_k^T lambda + M_k^T go   (+ g_{k-1} if k > 0)
 *     gz <- lambda
 * A failed step is a step whose DZ_k, DU_k are zero; everything else proceeds (with G_u = G_obs = NULL: gU[k] = 0 and nothing is added to gW, the
 * rule of dojo_rollout_adjoint_dev; with W = 0 the recursion for gU and gz IS that entry's).  mean and scale are frozen: no gradient is produced
 * for them, and the rounding of o_k is not differentiated.
 *
 * dojo_observation_jacobian_dev: maximal_to_minimal_jacobian (src/gradients/state.jl:9-56) of n * B states z [n][B][13Nb] (handle dtype) in one
 * launch over all (state, environment, joint) triples.  M is double [n][B][2nu][24], COMPACT and always fp64 (as dojo_get_mu is): row i is minimal
 * coordinate i in the order of dojo_maximal_to_minimal; columns 0..11 are the derivative w.r.t. the tangent coordinates of the PARENT body of the
 * joint that owns the row, columns 12..23 w.r.t. those of its CHILD body.  A joint on the origin has no parent columns: they are written as 0 and no
 * consumer reads them.  dojo_observation_jacobian: host pointers, z [B][13Nb] (n = 1).  Mechanisms with a kinematic loop: DOJO_ERR_UNSUPPORTED.
 *
 * dojo_rollout_policy_record_dev = dojo_rollout_policy_dev plus the record of dojo_rollout_record_dev (DZ [H][B][nx][nx], DU [H][B][nu][nx], device
 * layout).  Z, OBS, U_out, DZ, DU are required, status may be NULL.  It refuses what dojo_rollout_policy_dev and dojo_rollout_record_dev refuse.
 *
 * dojo_rollout_policy_adjoint_dev: the sweep above.  `policy` as for the forward call (bias and U_ff are not read); *a is host memory read during
 * the call, its members are device pointers in the handle dtype.  M = NULL: the library computes it from (z0, Z) into a workspace of the handle with
 * the kernel of dojo_observation_jacobian_dev (M[H] is computed and read only when G_obs is given).  per_env = 1: gW [B][na][nobs], gbias [B][na];
 * per_env = 0: gW [na][nobs], gbias [na], the sums over the batch (a second small kernel, summation order fixed by B alone).  Launches go on `stream`
 * only and nothing synchronizes (a workspace that has to GROW is replaced, which waits for the device once).  All arithmetic is fp64, outputs are
 * rounded once, no atomics: results are bit-identical from run to run and independent of the batch size and of an environment's place in the batch.
 * Refused before anything is launched, text on the handle -- DOJO_ERR_INVALID: what dojo_rollout_policy_dev refuses; NULL a, DZ, DU, OBS or G;
 * cot_space not 0 / 1; cot_space = 1 without Z; M = NULL without z0 and Z; DZ or DU not 16-byte aligned.  DOJO_ERR_UNSUPPORTED:
 * policy->contact_forces = 1 (the derivative of the previous step's impulses w.r.t. the state is not part of the record, and treating them as
 * constants would silently return something that is not the derivative); a sweep whose LDS need (4 nx + nu + 2 nobs + na (nobs + 1) doubles:
 * Ant 7 KB, Atlas 30 KB) exceeds 64 KB.
 *
 * dojo_rollout_policy_gradients (host pointers, the members of *policy included): uploads, records, sweeps, downloads Z [H][B][13Nb],
 * OBS [H+1][B][nobs], U_out [H][B][nu], status [H][B], gW, gbias, gU [H][B][nu], gz [B][nx] (each may be NULL).  G [H][B][nx | 13Nb] is required,
 * G_u [H][B][nu] and G_obs [H+1][B][nobs] may be NULL.  The record and M never cross PCIe; a record (plus M) that does not fit into the free device
 * memory: DOJO_ERR_INVALID with the byte count in the text, before any launch. */
typedef struct DojoPolicyAdjoint {
    const void* DZ;         /* [H][B][nx][nx] as recorded; required, 16-byte aligned                       */
    const void* DU;         /* [H][B][nu][nx] as recorded; required, 16-byte aligned                       */
    const void* OBS;        /* [H+1][B][nobs] as recorded; required                                        */
    const int32_t* status;  /* [H][B] or NULL (every step solved)                                          */
    const void* z0;         /* [B][13Nb]; needed when M is NULL                                            */
    const void* Z;          /* [H][B][13Nb]; needed when M is NULL, or cot_space = 1                       */
    const double* M;        /* [H+1][B][2nu][24] compact observation Jacobians, or NULL (computed)         */
    const void* G;          /* [H][B][nx] (cot_space 0) or [H][B][13Nb] (cot_space 1); required            */
    const void* G_u;        /* [H][B][nu] cotangent of U_out, or NULL                                      */
    const void* G_obs;      /* [H+1][B][nobs] cotangent of OBS, or NULL                                    */
    void* gW;               /* out: [Bw][na][nobs], or NULL                                                */
    void* gbias;            /* out: [Bw][na], or NULL                                                      */
    void* gU;               /* out: [H][B][nu] gradient w.r.t. U_ff, or NULL                               */
    void* gz;               /* out: [B][nx] gradient w.r.t. z0 in tangent coordinates, or NULL             */
    int32_t cot_space;      /* 0: G in tangent coordinates; 1: in state coordinates (as dojo_rollout_adjoint_dev) */
    int32_t reserved;
} DojoPolicyAdjoint;
int  dojo_observation_jacobian_dev(DojoHandle h, const void* z, int32_t n, double* M, void* stream);
int  dojo_observation_jacobian(DojoHandle h, const void* z, double* M);
int  dojo_rollout_policy_record_dev(DojoHandle h, const void* z0, const DojoPolicy* policy, int32_t H,
                                    void* Z, void* OBS, void* U_out, int32_t* status, void* DZ, void* DU, void* stream);
int  dojo_rollout_policy_adjoint_dev(DojoHandle h, const DojoPolicy* policy, int32_t H, const DojoPolicyAdjoint* a, void* stream);
int  dojo_rollout_policy_gradients(DojoHandle h, const void* z0, const DojoPolicy* policy, int32_t H, const void* G, int32_t cot_space,
                                   const void* G_u, const void* G_obs, void* Z, void* OBS, void* U_out, int32_t* status,
                                   void* gW, void* gbias, void* gU, void* gz);

/* Closed-loop rollouts with a network policy, forward and reverse mode: dojo_rollout_policy_dev and dojo_rollout_policy_adjoint_dev with a small tanh
 * MLP in place of the affine map -- first-order optimisation of a neural controller through the simulator in one call per direction.
 * csrc/dojo_mlp.hpp has the kernels.  Per environment b and step k, L = n_layers (1 .. DOJO_MLP_MAX_LAYERS), widths n_0 = nobs, hidden
 * n_1 .. n_{L-1}, n_L = na (the driven inputs: act_off .. act_off + na - 1), each >= 1:
 *
 *     o_k  = the observation of dojo_rollout_policy_dev (rounded once to the handle dtype -> OBS[k]; the policy consumes the ROUNDED value)
 *     h_0  = (o_k - mean) .* scale                                    fp64
 *     p_l  = b_l + W_l h_{l-1},   h_l = tanh(p_l)   l = 1 .. L-1      fp64;  h_1 .. h_{L-1} -> ACT[k][b]
 *     a    = b_L + W_L h_{L-1}                                        (no activation on the output layer)
 *     u    = U_ff[k][b];  u[act_off + i] += a_i                       rounded once -> U_out[k][b], read by step k
 *
 * theta: one flat vector of P = sum_l n_l (n_{l-1} + 1) entries in the handle dtype, layer after layer: W_l row-major [n_l][n_{l-1}], then b_l [n_l].
 * per_env = 1: theta [B][P]; per_env = 0: theta [P], shared.  ACT is double [H][B][nh], nh = n_1 + .. + n_{L-1}: fp64 whatever the handle dtype (as M
 * is); it is what the sweep reads, which therefore evaluates no tanh and repeats no forward pass.  With n_layers = 1, theta = [W | bias] and every
 * output of every entry below is bit-identical to the affine entry fed (W, bias).  tanh is the device library's fp64 tanh.  Every dot product is
 * summed in an order fixed by the widths alone; no atomics; results do not depend on the batch, the groups or per_env = 0 against theta given B times.
 *
 * dojo_rollout_mlp_dev (device pointers, the members of *policy included) mirrors dojo_rollout_policy_dev argument for argument, plus ACT; Z, OBS,
 * U_out, ACT, status may each be NULL.  dojo_rollout_mlp: host pointers.  dojo_rollout_mlp_record_dev = dojo_rollout_mlp_dev plus the record of
 * dojo_rollout_record_dev; Z, OBS, U_out, DZ, DU are required, and ACT with n_layers > 1.
 *
 * dojo_rollout_mlp_adjoint_dev: with the notation of dojo_rollout_policy_adjoint_dev (lambda, g_k, GU_k, GO_k, M_k, failed steps by select),
 *     gu = DU_k^T lambda + GU_k -> gU[k];   delta_L = gu[act_off .. act_off + na - 1]
 *     for l = L .. 1:   g b_l += delta_l;   g W_l += delta_l h_{l-1}^T;   delta_{l-1} = (W_l^T delta_l) .* (1 - h_{l-1}^2)   (no factor for l = 1)
 *     go = scale .* delta_0 + GO_k;   lambda = DZ_k^T lambda + M_k^T go (+ g_{k-1} if k > 0)
 * with h_0 formed from the recorded OBS[k] and h_l from the recorded ACT[k].  gtheta has the layout of theta: [B][P] (per_env = 1) or [P], the sum
 * over the batch (per_env = 0; a second small kernel, order fixed by B alone).  The P accumulators of an environment live in an fp64 workspace of
 * the handle ([B][P], grown on demand), each owned by one lane for the whole launch; fp64 throughout, outputs rounded once.  That workspace (like M's
 * and the affine sweep's) is ONE PER HANDLE and is read and written at every step of the sweep: sweeps on one handle must be ordered -- enqueue them on
 * one stream, or make the later one wait for the earlier; concurrent sweeps need a handle each.  mean and scale are
 * frozen; U_ff is not read.  dojo_rollout_mlp_gradients (host pointers): upload, record, sweep, download; the record, M and ACT
 * never cross PCIe, and the free-memory check of dojo_rollout_policy_gradients covers ACT and the workspace as well.
 *
 * Refused before anything is launched, text on the handle that names the entry point -- DOJO_ERR_INVALID: what the affine counterpart refuses (theta
 * in the place of W); n_layers outside 1 .. DOJO_MLP_MAX_LAYERS; a width < 1; width[0] != nobs; act_off + width[n_layers] > nu (na IS
 * width[n_layers]); n_layers > 1 with ACT = NULL in the record and adjoint entries.  DOJO_ERR_UNSUPPORTED: contact_forces = 1 in the adjoint and
 * gradients entries (the reason given above); a policy of 2^31 parameters or more; a policy whose LDS need exceeds 64 KB in either kernel --
 *     forward:  4 (nobs + nh) doubles                              (four environments per workgroup: h_0 and the activations)
 *     sweep:    4 nx + nu + 2 nobs + 2 wmax + nh doubles,  wmax = the largest width     (Ant, [28, 64, 64, 8]: 5 KB and 7.4 KB)
 * Not part of it: other activations, output squashing or clamping, gradients w.r.t. mean and scale, contact observations in reverse mode. */
#define DOJO_MLP_MAX_LAYERS 4
typedef struct DojoMlpPolicy {
    const void* theta;    /* [Bw][P], handle dtype; required                                            */
    const void* mean;     /* [nobs] or NULL (zeros): shared by all environments                         */
    const void* scale;    /* [nobs] or NULL (ones)                                                      */
    const void* U_ff;     /* [H][B][nu] or NULL (zeros)                                                 */
    int32_t per_env;      /* 1: Bw = B (one policy per environment); 0: Bw = 1 (shared)                 */
    int32_t act_off;      /* the policy drives inputs act_off .. act_off + width[n_layers] - 1          */
    int32_t n_layers;     /* L: 1 .. DOJO_MLP_MAX_LAYERS (1: the affine policy)                         */
    int32_t width[DOJO_MLP_MAX_LAYERS + 1];   /* n_0 = nobs, n_1 .. n_{L-1}, n_L = na; entries past L are not read */
    int32_t contact_forces;/* nobs = 2 nu + (contact_forces ? Nc : 0), as dojo_observe_dev              */
    int32_t contact_init; /* as DojoPolicy                                                              */
    int32_t reserved;
} DojoMlpPolicy;
typedef struct DojoMlpAdjoint {
    const void* DZ;         /* [H][B][nx][nx] as recorded; required, 16-byte aligned                       */
    const void* DU;         /* [H][B][nu][nx] as recorded; required, 16-byte aligned                       */
    const void* OBS;        /* [H+1][B][nobs] as recorded; required                                        */
    const double* ACT;      /* [H][B][nh] as recorded; required with n_layers > 1                          */
    const int32_t* status;  /* [H][B] or NULL (every step solved)                                          */
    const void* z0;         /* [B][13Nb]; needed when M is NULL                                            */
    const void* Z;          /* [H][B][13Nb]; needed when M is NULL, or cot_space = 1                       */
    const double* M;        /* [H+1][B][2nu][24] compact observation Jacobians, or NULL (computed)         */
    const void* G;          /* [H][B][nx] (cot_space 0) or [H][B][13Nb] (cot_space 1); required            */
    const void* G_u;        /* [H][B][nu] cotangent of U_out, or NULL                                      */
    const void* G_obs;      /* [H+1][B][nobs] cotangent of OBS, or NULL                                    */
    void* gtheta;           /* out: [Bw][P], or NULL                                                       */
    void* gU;               /* out: [H][B][nu] gradient w.r.t. U_ff, or NULL                               */
    void* gz;               /* out: [B][nx] gradient w.r.t. z0 in tangent coordinates, or NULL             */
    int32_t cot_space;      /* 0: G in tangent coordinates; 1: in state coordinates                        */
    int32_t reserved;
} DojoMlpAdjoint;
int  dojo_rollout_mlp_dev(DojoHandle h, const void* z0, const DojoMlpPolicy* policy, int32_t H,
                          void* Z, void* OBS, void* U_out, double* ACT, int32_t* status, void* stream);
int  dojo_rollout_mlp(DojoHandle h, const void* z0, const DojoMlpPolicy* policy, int32_t H,
                      void* Z, void* OBS, void* U_out, int32_t* status);
int  dojo_rollout_mlp_record_dev(DojoHandle h, const void* z0, const DojoMlpPolicy* policy, int32_t H,
                                 void* Z, void* OBS, void* U_out, double* ACT, int32_t* status, void* DZ, void* DU, void* stream);
int  dojo_rollout_mlp_adjoint_dev(DojoHandle h, const DojoMlpPolicy* policy, int32_t H, const DojoMlpAdjoint* a, void* stream);
int  dojo_rollout_mlp_gradients(DojoHandle h, const void* z0, const DojoMlpPolicy* policy, int32_t H, const void* G, int32_t cot_space,
                                const void* G_u, const void* G_obs, void* Z, void* OBS, void* U_out, int32_t* status,
                                void* gtheta, void* gU, void* gz);

/* Batched iLQR: the Riccati backward pass in minimal coordinates (csrc/dojo_riccati.hpp).  The reference's examples/trajectory_optimization run
 * IterativeLQR over get_minimal_gradients! (src/gradients/state.jl:183-217); this is IterativeLQR's backward pass for B environments at once, over the
 * Jacobians H calls of dojo_minimal_gradients_dev leave on the device (jx -> A + k B n n, ju -> Bm + k B n nu: they fill the record in place).
 * n = 2 nu; the policy drives the inputs act_off .. act_off + na - 1 as in DojoPolicy, m = na.  Per environment b, A_k = A[k][b] [n x n] row-major,
 * B_k = the columns act_off .. act_off + na - 1 of Bm[k][b] [n x nu] row-major:
 *     Vx <- lx_H;  Vxx <- lxx_H;  dV <- (0, 0);  fail <- 0
 *     for k = H-1 .. 0:
 *         if status && status[k][b] != 0:  A_k, B_k are NOT read (they may be NaN) and count as zero   (nothing flows through a failed step)
 *         Qx  = lx_k + A^T Vx            Qu  = lu_k + B^T Vx
 *         Qxx = lxx_k + A^T Vxx A        Qux = lux_k + B^T Vxx A  (lux NULL = 0)       Quu = luu_k + B^T Vxx B
 *         Qreg = Quu + mu[b] I           (mu NULL = 0)
 *         Cholesky Qreg = L L^T; a pivot that is not > 0 or not finite:  fail <- k + 1, stop this environment
 *         kff_k = -Qreg^-1 Qu            K_k = -Qreg^-1 Qux
 *         dV[0] += kff^T Qu              dV[1] += 1/2 kff^T Quu kff      (Quu, not Qreg: the expected change for step length a is  a dV[0] + a^2 dV[1])
 *         Vx  = Qx  + K^T Quu kff + K^T Qu  + Qux^T kff
 *         Vxx = Qxx + K^T Quu K   + K^T Qux + Qux^T K;   Vxx <- (Vxx + Vxx^T) / 2
 * Outputs: K [H][B][na][n], kff [H][B][na], fail [B] (int32), and -- each may be NULL -- dV [B][2], Vx [B][n], Vxx [B][n][n] (the value function at k = 0).
 * lxx_k and luu_k are symmetric matrices: the kernel uses their symmetric parts.  On failure at step k: K, kff of the steps <= k are written as zeros, the steps
 * above k keep what was computed, dV, Vx, Vxx of that environment are written as zeros.  Every element of every given output is written in every case; a NaN in
 * one environment's Jacobians ends as that environment's `fail` and nowhere else.
 * Inputs are in the handle dtype and converted on load; every product and sum is fp64, the state of the recursion stays fp64 between the steps, outputs are
 * rounded once.  No atomics; the summation order is fixed by (n, na) alone: results are bit-identical from run to run and do not depend on B or on the
 * environment's place in the batch.
 * dojo_riccati_dev: device pointers, ONE launch on `stream`, no synchronization.  dojo_riccati: host pointers, staged like the other host entries.  The
 * struct is host memory, read during the call.
 * DOJO_ERR_INVALID (text on the handle, nothing launched): H < 1; a NULL required member (A, Bm, lx, lu, lxx, luu, K, kff, fail); nu = 0; na < 1,
 * act_off < 0 or act_off + na > nu.  DOJO_ERR_UNSUPPORTED: a mechanism with a kinematic loop (as dojo_minimal_gradients_dev); a shape the kernel's plan
 * cannot hold -- more than 64 KB of LDS (8 (n (n + 1) / 2 + max(32 (n + na), na n + 2 na^2) + 2 n + 4 na + 8) bytes: Ant (28, 8) 13 KB, Atlas (72, 30) 55 KB),
 * n + na > 110 (the accumulators of the lower triangle of [Qxx Qxu; Qux Quu] live in registers), na > 64 -- with the byte count in the text.
 * Not part of it: the forward pass and the linearization along it (each is one call of the rollout in minimal coordinates of include/dojo_hip_trajopt.h,
 * whose controller takes K and kff as they are written here), control limits (the box variant of this pass and of that rollout: include/dojo_hip_limits.h),
 * costs shared across the batch or given as diagonals, second-order dynamics terms (DDP), constraints (augmented Lagrangian), kinematic loops.
 * (The line search that follows this pass -- all its step lengths as one rollout, the acceptance test as one kernel that reads this pass's dV --:
 * include/dojo_hip_linesearch.h.) */
typedef struct DojoRiccati {
    const void* A;      /* [H][B][n][n]   row-major, jx of dojo_minimal_gradients_dev per step */
    const void* Bm;     /* [H][B][n][nu]  row-major, ju ...; columns act_off .. act_off+na-1 are read */
    const int32_t* status; /* [H][B] or NULL */
    const void *lx, *lu, *lxx, *luu, *lux; /* [H+1][B][n], [H][B][na], [H+1][B][n][n], [H][B][na][na], [H][B][na][n] or NULL */
    const void* mu;     /* [B] or NULL */
    void *K, *kff; int32_t* fail;          /* required */
    void *dV, *Vx, *Vxx;                   /* each may be NULL */
    int32_t act_off, na;
} DojoRiccati;
int  dojo_riccati_dev(DojoHandle h, int32_t H, const DojoRiccati* r, void* stream);
int  dojo_riccati(DojoHandle h, int32_t H, const DojoRiccati* r);

/* get_state(environment) of DojoEnvironments (environments.jl:100-102; quadruped_sampling.jl:67-72): the minimal state
 * of the mechanism, and with contact_forces != 0 the normal impulse of every contact of the last step clamped to
 * [-1, 1] behind it (get_state(::AntARS), ant_ars.jl:72-80).  obs [B, 2*nu (+ Nc)].
 * dojo_observe reads the state the last dojo_step / dojo_step_minimal / dojo_rollout left on the handle; the device
 * variant takes that state z [B, 13Nb] explicitly (the z_next of the step enqueued before it on `stream`; NULL = the
 * state kept on the handle, e.g. after dojo_step_minimal_dev). */
int  dojo_observe(DojoHandle h, void* obs, int32_t contact_forces);
int  dojo_observe_dev(DojoHandle h, const void* z, void* obs, int32_t contact_forces, void* stream);

/* get_contact_gradients(mechanism)  src/gradients/contact.jl:1-55  (SURVEY.md §8f-3): the Jacobian of the next state
 * [x3; v25; phi3; omega25] w.r.t. the contact data, 5 per contact [friction_coefficient, contact_radius, contact_origin(3)],
 * at the solution of the last differentiable step (dojo_step(..., with_gradient = 1) / dojo_step_dev with dz, du).
 * dc [B, 12Nb, 5Nc] row-major (host variant); the device variant takes the same z, u as that step and writes
 * dc[B][5Nc columns][12Nb rows] (column-major per environment, like dz).  Quad mappings (<= 32 bodies). */
int  dojo_contact_gradients(DojoHandle h, void* dc);
int  dojo_contact_gradients_dev(DojoHandle h, const void* z, const void* u, void* dc, void* stream);

/* Minimal <-> maximal coordinates.  x [B, 2*nu]: per joint, in mechanism.joints order,
 * [dx(nu_tra); dtheta(nu_rot); dv(nu_tra); domega(nu_rot)].
 *   minimal_to_maximal(mechanism, x)   src/mechanism/state.jl:9-22  (+ src/joints/minimal.jl:160-232)
 *   maximal_to_minimal(mechanism, z)   src/mechanism/state.jl:44-66
 *   step_minimal_coordinates!(mechanism, x, u)   src/simulation/step.jl:42-60   (x -> z -> step! -> z' -> x') */
int  dojo_minimal_to_maximal(DojoHandle h, const void* x, void* z);
int  dojo_maximal_to_minimal(DojoHandle h, const void* z, void* x);
int  dojo_step_minimal(DojoHandle h, const void* x, const void* u, void* x_next, int32_t* status, int32_t* iters);
int  dojo_minimal_to_maximal_dev(DojoHandle h, const void* x, void* z, void* stream);
int  dojo_maximal_to_minimal_dev(DojoHandle h, const void* z, void* x, void* stream);
int  dojo_step_minimal_dev(DojoHandle h, const void* x, const void* u, void* x_next,
                           int32_t* status, int32_t* iters, void* stream);

/* get_minimal_gradients!(mechanism, y, u; opts)  src/gradients/state.jl:183-217: one step in minimal coordinates and the
 * Jacobians of x_next w.r.t. x and u, = max_to_min_jacobian * (jacobian_state | jacobian_control) * min_to_max_jacobian
 * (src/gradients/state.jl:9-56, 136-181).  jx [B, 2nu, 2nu], ju [B, 2nu, nu], row-major.  With DOJO_GRAD_REFERENCE the
 * two coordinate Jacobians are evaluated where the reference evaluates them (post-update_state! states). */
int  dojo_minimal_gradients(DojoHandle h, const void* x, const void* u, void* x_next, int32_t* status, int32_t* iters,
                            void* jx, void* ju);
int  dojo_minimal_gradients_dev(DojoHandle h, const void* x, const void* u, void* x_next, int32_t* status, int32_t* iters,
                                void* jx, void* ju, void* stream);

/* timing helper for bench.py: average duration in ms of the last `n` launches of the
 * step kernel measured with hipEvents on the launch stream (roofline.achieved).
 * With environment groups (dojo_set_groups / the library's default for B >= 512) every group is a launch of its own with its own
 * event pair: dojo_last_kernel_ms / dojo_last_kernel_times then report the LAST GROUP's kernels (1/groups of the batch), and
 * dojo_kernel_time_totals sums intervals that overlap in time and counts `groups` launches per step.  For the duration of a kernel
 * over the whole batch call dojo_set_groups(h, 1) first (what bench.py does for its roofline leg). */
int  dojo_last_kernel_ms(DojoHandle h, double* ms);
/* the same, split by kernel: the step kernel (Newton loop: step!/mehrotra!) and the IFT kernel (the
 * back-solves of get_maximal_gradients!, src/gradients/state.jl:78-126; 0 when not requested) */
int  dojo_last_kernel_times(DojoHandle h, double* step_ms, double* ift_ms);
/* totals over all timed launches since the last reset (the events are kept in a ring, so timing never makes the
 * host wait inside a rollout loop): summed kernel durations in ms and the number of step launches */
int  dojo_kernel_time_totals(DojoHandle h, double* step_ms, double* ift_ms, int64_t* launches, int32_t reset);

#ifdef __cplusplus
}
#endif
#endif /* DOJO_HIP_H */
