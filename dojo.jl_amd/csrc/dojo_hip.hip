// dojo_hip.hip -- libdojo_hip.so: host side of the C ABI of include/dojo_hip.h.  Host code only: the step and IFT kernels are dojo_kernels.hip's,
// every other kernel family has a header of its own (dojo_coord_kernels.hpp, dojo_adjoint.hpp, dojo_policy.hpp, ...) and a launch_*<TIO> here;
// the one kernel in this file is the scheduler's dispatch_order_kernel.
//
// One wavefront = 64/S environments x S supernodes (dojo_device.hpp).  One workgroup = one
// wavefront (64 threads), so a batch of B environments launches ceil(B*S/64) workgroups --
// 1024 for Ant at B = 4096, i.e. one wave per SIMD on the 256 CUs (>> 256 workgroups, and the
// kernel needs no LDS, so placement across the 8 XCDs is irrelevant: nothing is shared).
// There is deliberately no CPU fallback in this library: without a gfx950 device dojo_create
// fails with DOJO_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>
#include "dojo_host.hpp"
#include "dojo_coord_kernels.hpp"
#include "dojo_adjoint.hpp"
#include "dojo_policy.hpp"
#include "dojo_policy_adjoint.hpp"
#include "dojo_mlp.hpp"
#include "dojo_data_adjoint.hpp"
#include "dojo_tangent.hpp"
#include "dojo_riccati.hpp"
#include "dojo_tracking.hpp"
#include "dojo_linesearch.hpp"
#include "../../include/dojo_hip_constraints.h"      // (includes dojo_hip_limits.h, which includes dojo_hip_trajopt.h)
#include "../../include/dojo_hip_linesearch.h"       // (the fifth: the fan rollout and the selection kernel of a side-by-side line search)
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <map>
#include <vector>
#include <deque>
#include <algorithm>
#include <mutex>
#include <dlfcn.h>

struct DojoSim;
namespace {

// Error text: one process-wide string behind a mutex (dojo_last_error: what the last failing call on ANY thread said -- a
// Julia task may migrate between the failing @ccall and the query, so it must not be thread-local) and a copy on the handle
// the failing entry point was called with (dojo_handle_error: per handle).
void handle_set_error(::DojoSim* s, const std::string& m);
thread_local ::DojoSim* t_handle = nullptr;            // handle of the entry point running on this thread
struct ErrSink {
    std::mutex m; std::string last; std::string ret;
    ErrSink& operator=(const std::string& v) { { std::lock_guard<std::mutex> g(m); last = v; } if (t_handle) handle_set_error(t_handle, v); return *this; }
    ErrSink& operator=(const char* v) { return *this = std::string(v); }
    const char* c_str() { std::lock_guard<std::mutex> g(m); ret = last; return ret.c_str(); }
} g_err;
struct Enter { ::DojoSim* prev; explicit Enter(::DojoSim* s) : prev(t_handle) { t_handle = s; } ~Enter() { t_handle = prev; } };

// kernel launchers, one per object file of dojo_kernels.hip: dojo_launch_<abi type>_<max contacts per body>_<quad>
extern "C" {
#define DJ_DECL(n) int n(const void*, int, void*, int, void*);
DJ_DECL(dojo_launch_float_1_1) DJ_DECL(dojo_launch_float_4_1) DJ_DECL(dojo_launch_float_8_1)
DJ_DECL(dojo_launch_double_1_1) DJ_DECL(dojo_launch_double_4_1) DJ_DECL(dojo_launch_double_8_1)
DJ_DECL(dojo_launch_float_4_0) DJ_DECL(dojo_launch_float_8_0) DJ_DECL(dojo_launch_double_4_0) DJ_DECL(dojo_launch_double_8_0)
DJ_DECL(dojo_launch_float_4_2) DJ_DECL(dojo_launch_double_4_2) DJ_DECL(dojo_launch_float_1_2) DJ_DECL(dojo_launch_double_1_2)
// the builds with translational springs / dampers (-DDJ_TSD=1): single-wavefront quad mapping, <= 4 contacts per body
DJ_DECL(dojo_launch_tsd_float_1_1) DJ_DECL(dojo_launch_tsd_float_4_1) DJ_DECL(dojo_launch_tsd_double_1_1) DJ_DECL(dojo_launch_tsd_double_4_1)
DJ_DECL(dojo_launch_tsd_float_4_0) DJ_DECL(dojo_launch_tsd_float_8_0) DJ_DECL(dojo_launch_tsd_double_4_0) DJ_DECL(dojo_launch_tsd_double_8_0)
DJ_DECL(dojo_launch_gen_float_4_0) DJ_DECL(dojo_launch_gen_float_8_0) DJ_DECL(dojo_launch_gen_double_4_0) DJ_DECL(dojo_launch_gen_double_8_0)
DJ_DECL(dojo_launch_lin_float_1_1) DJ_DECL(dojo_launch_lin_float_4_1) DJ_DECL(dojo_launch_lin_double_1_1) DJ_DECL(dojo_launch_lin_double_4_1)     // LinearContact builds
DJ_DECL(dojo_launch_lin_float_4_0) DJ_DECL(dojo_launch_lin_float_8_0) DJ_DECL(dojo_launch_lin_double_4_0) DJ_DECL(dojo_launch_lin_double_8_0)
DJ_DECL(dojo_launch_ss_float_1_1) DJ_DECL(dojo_launch_ss_double_1_1)     // body-body contacts (-DDJ_SS=1): single-wavefront quad mapping, <= 1 contact per body, forward only
#define DJ_CDECL(n) int n(const void*, int, void*);
DJ_CDECL(dojo_launch_cgrad_float_1_1) DJ_CDECL(dojo_launch_cgrad_float_4_1) DJ_CDECL(dojo_launch_cgrad_float_8_1)
DJ_CDECL(dojo_launch_cgrad_double_1_1) DJ_CDECL(dojo_launch_cgrad_double_4_1) DJ_CDECL(dojo_launch_cgrad_double_8_1)
DJ_CDECL(dojo_launch_cgrad_float_4_2) DJ_CDECL(dojo_launch_cgrad_double_4_2) DJ_CDECL(dojo_launch_cgrad_float_1_2) DJ_CDECL(dojo_launch_cgrad_double_1_2)
DJ_CDECL(dojo_launch_cgrad_tsd_float_1_1) DJ_CDECL(dojo_launch_cgrad_tsd_float_4_1) DJ_CDECL(dojo_launch_cgrad_tsd_double_1_1) DJ_CDECL(dojo_launch_cgrad_tsd_double_4_1)
#undef DJ_DECL
}

#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { g_err = std::string(#x) + ": " + hipGetErrorString(e_); return DOJO_ERR_DEVICE; } } while (0)
#define TRY(x) do { int rc_ = (x); if (rc_ != DOJO_OK) return rc_; } while (0)      // (a failing call of the library's own has set the error text)

// A step with the iteration cap in force (dojo_set_iteration_cap) is launched in phases: the step kernel of every environment group
// (PH_MAIN), each followed on its stream by the IFT kernel of the workgroups it finished (PH_GRAD); behind the step kernels of ALL groups,
// on a stream of its own, the continuation of the listed workgroups and their IFT (PH_CONT, once over the whole batch).  PH_ALL = no cap:
// step kernel + IFT kernel in one go.
enum { PH_ALL = 0, PH_MAIN = 1, PH_GRAD = 2, PH_CONT = 3 };
// What a launch of the step (and IFT) kernels is told: the caller's batch-level device buffers (null = not wanted; the solution buffers are the handle's),
// the environments [env0, env0 + nenv) and their stream (env0: a multiple of the environments per wavefront), and how the kernels are run
struct StepIO { const void *z, *u; void* z_next; int *status, *iters; void *dz, *du, *dc, *storage; };
struct Span { size_t env0; int nenv; hipStream_t stream; };
// What a rollout (rollout_core) is told: device arrays over the H steps, null = not given / not wanted
struct Controller;
struct RolloutIO {
    const void* z0 = nullptr;               // [B][nz] the initial state (required)
    const void* U = nullptr;                // [H][B][nu] pre-sampled controls; with a controller: its feed-forward term
    void* Z = nullptr;                      // [H][B][nz] the state behind every step (null: the last one alone, in the handle's d_zn)
    int32_t* status = nullptr;              // [H][B]
    void* storage = nullptr;                // [H][B][Nb][25] save_to_storage! rows of every solved step
    void *DZ = nullptr, *DU = nullptr;      // [H][B][nx][nx] / [H][B][nu][nx] the IFT Jacobians of every step, in the device layout of dojo_step_dev (dojo_rollout_record_dev)
    void* DC = nullptr;                     // [H][B][5Nc][nx] (with DZ) the contact-data columns of every step: the step launch of a group is followed directly, on the same span and stream,
                                            // by the contact-data IFT kernel of dojo_contact_gradients_dev, which reads the hand-off record that step just left for exactly those environments
    const Controller* controller = nullptr; // closed loop (checked by the caller): the controls of step k are made on the group's stream, directly in front of the step, by the policy kernel ...
    void* OBS = nullptr;                    // ... [H+1][B][nobs] what it saw
    void* U_out = nullptr;                  // ... [H][B][nu] what it made (null: one [B][nu] buffer of the handle, a group's launches being serial)
    // A rollout in minimal coordinates (the tracking controller, dojo_rollout_minimal_dev): z0 is the minimal state [B][2nu], OBS is X [H+1][B][2nu], Z is not recorded -- the
    // controller re-projects X[k] into the handle's d_z, the step goes from there into d_zn, as dojo_step_minimal_dev does it -- and with
    void *A = nullptr, *Bm = nullptr;       // ... [H][B][2nu][2nu], [H][B][2nu][nu] the chain of dojo_minimal_gradients_dev runs behind every step of a group, on its span and stream
};
struct Mode {
    int phase;
    int* slot;                         // timed launches: where a PH_ALL / PH_MAIN launch puts the timing slot it took, and the PH_GRAD launch of the same group finds it; null = not timed
    bool cap_lists, chained;           // phased launches: with the iteration cap's lists (pipelined groups launch the two kernels apart without them); one of a group's steps launched back to back (rollout_core)
    size_t groups; int rec;            // environment groups of the step this launch belongs to; the step -> IFT hand-off record in use (DojoSim::sol_cur: state between calls -- a launch is told it)
    Mode with(int phase_, int* slot_) const { Mode m = *this; m.phase = phase_; m.slot = slot_; return m; }
};
// the environment groups of a batch: NG groups of `per` environments (a multiple of 64: whole wavefronts for every mapping), the last ones shorter or empty
struct Partition {
    size_t B, NG, per;
    explicit Partition(size_t B_ = 0, size_t NG_ = 1) : B(B_), NG(NG_), per(((B_ + NG_ - 1) / NG_ + 63) / 64 * 64) {}
    size_t groups() const { return std::min(NG, (B + per - 1) / per); }      // the non-empty ones
    Span span(size_t gi, hipStream_t st) const { return Span{gi * per, (int)std::min(per, B - gi * per), st}; }
    bool operator!=(const Partition& o) const { return NG != o.NG || per != o.per; }
};

} // namespace

struct DojoSim {
    dj::HostModel M;
    DojoSolverOptions opts;
    int B = 0, dtype = 0, device = 0, grad_mode = DOJO_GRAD_REFERENCE;
    size_t w = 8;                       // bytes per scalar
    void* d_tsd = nullptr;       // translational springs / dampers per supernode (mechanisms that have them)
    void* d_mlim = nullptr;      // joint limits on several coordinates per supernode (mechanisms that have them)
    void* d_cuts = nullptr;      // loop-closing joints (mechanisms with kinematic loops)
    void* d_cutws = nullptr;     // [B][dj::CUTWS] doubles: per-environment workspace of the cut elements (KernelArgs::cutws)
    void* d_nodes = nullptr; void* d_contacts = nullptr; int* d_order = nullptr;   // tables; bodies in root -> leaves order
    void *d_x = nullptr, *d_xn = nullptr;   // minimal-coordinate buffers of the host-pointer entry points
    void *d_cz = nullptr;                   // maximal-state scratch of dojo_minimal_to_maximal / dojo_maximal_to_minimal (d_z stays the state of the last step)
    void *d_jf = nullptr;                   // dojo_step_impulses: body impulses folded into the external-force slot
    double *d_mu = nullptr;                 // [B] mechanism.μ at the end of the last step (dojo_get_mu)
    double *d_diag = nullptr;               // [B][2] diagnostics of the last step's final linearization (dojo_get_diagnostics)
    void *d_jm = nullptr, *d_jt = nullptr, *d_jb = nullptr;   // get_minimal_gradients!: min->max Jacobian, dz * that, max->min blocks (fp64)
    // internal device buffers used by the host-pointer entry points
    const void* fext = nullptr;                     // device [B,6Nb] external forces applied by every step, or null (dojo_set_external_force)
    void *d_fext = nullptr, *d_res = nullptr, *d_z = nullptr, *d_u = nullptr, *d_zn = nullptr, *d_vel = nullptr, *d_jimp = nullptr, *d_csg = nullptr, *d_dz = nullptr, *d_du = nullptr;
    std::vector<hipStream_t> gstreams; std::vector<hipEvent_t> gevents; hipEvent_t fork_event = nullptr;   // environment groups (rollouts, dojo_step_dev)
    int groups = -1;                    // environment groups of dojo_step_dev: -1 = chosen from the batch size, 1 = one launch on the caller's stream
    int async = 0; bool pending = false;   // dojo_set_async: 1 = dojo_step_dev returns without joining the groups into the caller's stream; 2 = ... and the IFT of a
                                        // group's step runs on a second stream of the group, next to its NEXT step kernel (two hand-off records in turn)
    std::vector<hipStream_t> gstreams2; std::vector<hipEvent_t> gevents2, grad_done[2];   // pipelined groups: the IFT streams, their join events, "IFT that read record p is through"
    void* d_sol2 = nullptr; int sol_cur = 0;                                              // the second hand-off record; the one in use
    Partition last_part;                   // environment-group partition of the last grouped dojo_step_dev (per-group chaining assumes it repeats)
    void* d_sol = nullptr;              // step kernel -> IFT kernel hand-off (converged solution, fp64)
    void* d_fac = nullptr;              // ... and the final supernode factors (quad mapping; explicit-inverse consumers only)
    void* d_lu = nullptr;               // the IFT kernel's LU-form factors between its phases (quad mapping)
    void* d_blk = nullptr;              // un-factored supernode rows of the environments whose solves are refined (quad mapping, DJ_REFINE)
    void* d_msg = nullptr;              // quad mapping: messages of the IFT up-sweep to the roots (KernelArgs::msg)
    void* d_ypark = nullptr;            // fp32 ABI, quad mapping: the IFT's forward-substituted right-hand sides between its two sweeps, in fp64
    int* d_flag = nullptr;              // [B] environments the plain step kernel deferred to the refining kernels
    double refine_w = -1.0;             // refine once max γ/s of an environment exceeds this (dojo_set_refinement); < 0: chosen from the tolerances
    int *d_status = nullptr, *d_iters = nullptr;
    void* d_pu = nullptr;               // [B][nu] the controls of a closed-loop rollout whose caller records none (dojo_rollout_policy_dev)
    int *d_touch_ptr = nullptr, *d_touch_ent = nullptr;    // per body, the (row, half) entries of the observation Jacobian that touch it (CSR; dojo_policy_adjoint.hpp)
    void* d_pM = nullptr; size_t pM_bytes = 0;             // [H+1][B][2nu][24] fp64: the observation Jacobians of a closed-loop sweep whose caller passes none (grown on demand)
    double* d_pacc = nullptr;                              // [B][na (nobs + 1)] fp64: per-environment gW / gbias of a shared policy, in front of the reduction
    size_t pacc_bytes = 0;
    double* d_dacc = nullptr; size_t dacc_bytes = 0;       // [B][5Nc] fp64: per-environment contact-data gradients in front of the reduction (dojo_data_adjoint.hpp)
    double* d_macc = nullptr; size_t macc_bytes = 0;       // [B][P] fp64: the accumulators of the MLP sweep between its steps, and in front of the reduction (dojo_mlp.hpp)
    // iteration cap + continuation kernel (dojo_set_iteration_cap; dojo_device.hpp Globals::iter_cap)
    int iter_cap = -1;                  // < 0: automatic (DOJO_DEFAULT_ITERATION_CAP where the continuation kernel exists), 0: off, > 0: as given
    void* d_resume = nullptr;           // [B][CARRY_PER_ENV] loop scalars of the solves the step kernel left unfinished
    int *d_cont_list = nullptr, *d_cont_count = nullptr;   // [workgroups of the batch] the continuation list (batch-level workgroup indices), [1] its length
    int *d_cstat = nullptr;             // [B] status buffer of launches whose caller passed none (the continuation kernel reads it)
    hipStream_t cstream = nullptr; hipEvent_t cont_event = nullptr, allmain_event = nullptr; std::vector<hipEvent_t> main_events;   // the continuation's stream; "step kernel done" per group
    // dispatch order of the step kernel (dojo_set_dispatch_order): 0 off, 1 where a launch has more workgroups than the GPU holds at once and the step is
    // joined into the caller's stream (the step then waits for its last wavefront), 2 always
    int dispatch_mode = 1, sm_count = 0;
    int *d_dispatch = nullptr, *d_liters = nullptr;        // [workgroups of the batch] the permutations, one segment per launch; [B] iteration counts when the caller passes no buffer
    std::map<size_t, int> dispatch_have;                   // first workgroup of a segment -> environments of the launch whose permutation it holds
    std::vector<int> group_slot;        // timing slot of the phased launches of an environment group (PH_MAIN -> PH_GRAD)
    std::vector<void*> owned;           // device memory of this handle (ensure), freed by dojo_destroy
    size_t* measure = nullptr;          // not null: ensure / ensure_at_least add what they would allocate to it, and allocate nothing (Measuring)
    bool have_grad = false, have_solution = false, have_u = false;
    std::string err; std::mutex err_m;  // text of the last failure of a call on this handle (dojo_handle_error)
    void* comm = nullptr; int comm_rank = 0, comm_world = 1;   // RCCL communicator of this handle's process group (dojo_comm_init)
    // kernel timing: a ring of event triples (launch begin / between the step and the IFT kernel / end), so that
    // timed launches never make the host wait; totals are accumulated when a slot is reused or queried
    struct Ev3 { hipEvent_t a = nullptr, m = nullptr, b = nullptr; bool has_mid = false, used = false; int n = 1; };
    std::vector<Ev3> ring; size_t ring_next = 0; int last_slot = -1;
    double acc_step_ms = 0, acc_ift_ms = 0; long long acc_n = 0;
};

namespace {
void handle_set_error(::DojoSim* s, const std::string& m) { std::lock_guard<std::mutex> g(s->err_m); s->err = m; }

// The ABI has two scalar types.  This is the one place that picks a template argument from the handle's: f is called with a float or a double,
// `by_dtype(s, [&](auto t) { return launch_x<decltype(t)>(s, ...); })`.
template <class F> int by_dtype(const DojoSim* s, F&& f) { return s->dtype == DOJO_DTYPE_F32 ? f(float()) : f(double()); }

// What every entry that works in minimal coordinates refuses, under its own name: a mechanism with a kinematic loop
int refuse_minimal(const DojoSim* s, const char* who, const char* note = " (the reference sets them with exclude_ids)") {
    if (!s->M.has_loop) return DOJO_OK;
    g_err = std::string(who) + ": the minimal coordinates of a mechanism with a kinematic loop are not those of a tree traversal" + note + ": not supported";
    return DOJO_ERR_UNSUPPORTED;
}

// dojo_set_dispatch_order: the permutation the NEXT step kernel of these workgroups hands its hardware workgroups out by -- a counting sort of
// the launch's workgroups by the Newton iterations their environments took in this step, longest first (a solve that was long stays long for
// a while: the same contacts are closing).  One workgroup; the order inside a bucket is whatever the atomics give (results do not depend on it:
// every environment is computed by the same program wherever it runs).  E = environments per workgroup.
__global__ void __launch_bounds__(1024) dispatch_order_kernel(const int* iters, int nenv, int E, int nwg, int* order) {
    __shared__ int cnt[64];
    const int t = (int)threadIdx.x;
    if (t < 64) cnt[t] = 0;
    __syncthreads();
    auto bucket = [&](int wg) { int k = 0; for (int e = 0; e < E; ++e) { const int env = wg * E + e; if (env < nenv) k = max(k, iters[env]); } return 63 - min(max(k, 0), 63); };
    for (int wg = t; wg < nwg; wg += 1024) atomicAdd(&cnt[bucket(wg)], 1);
    __syncthreads();
    if (t == 0) { int a = 0; for (int b = 0; b < 64; ++b) { const int c = cnt[b]; cnt[b] = a; a += c; } }
    __syncthreads();
    for (int wg = t; wg < nwg; wg += 1024) order[atomicAdd(&cnt[bucket(wg)], 1)] = wg;
}

// what an allocation takes from the device: whole 4096-byte granules, at least 8 bytes
size_t granules(size_t bytes) { return (std::max<size_t>(bytes, 8) + 4095) / 4096 * 4096; }
// While one lives, the handle measures: the code that allocates its workspaces runs as usual, and every buffer it would have to allocate adds its size to
// `bytes` instead -- what a call is going to take is totalled by the lines that take it
struct Measuring {
    DojoSim* s; size_t bytes = 0;
    explicit Measuring(DojoSim* s_) : s(s_) { s->measure = &bytes; }
    ~Measuring() { s->measure = nullptr; }
    Measuring(const Measuring&) = delete; Measuring& operator=(const Measuring&) = delete;
};
// device memory of the handle, allocated on first use and freed with the handle
int ensure(DojoSim* s, void** p, size_t bytes) {
    if (*p) return DOJO_OK;
    if (s->measure) { *s->measure += granules(bytes); return DOJO_OK; }
    HIPCHK(hipMalloc(p, bytes ? bytes : 8));
    s->owned.push_back(*p);
    return DOJO_OK;
}
#define ENSURE(p, ...) TRY(ensure(s, (void**)&(p), (__VA_ARGS__)))

template <class T>
int upload_tables(DojoSim* s) {   // tables are stored in the state precision (fp64)
    std::vector<dj::NodeP<T>> nodes; for (auto& n : s->M.nodes) nodes.push_back(dj::cast_node<T>(n));
    // one extra entry for the idle supernode slots of a workgroup: node 0 without contacts (a slot that kept node 0's
    // contacts would write the same contact-pool rows as the real node 0 in the two-wavefront mapping)
    { dj::NodeP<T> idle = nodes[0]; idle.ncontact = 0; for (int i = 0; i < 8; ++i) idle.contact[i] = 0; nodes.push_back(idle); }
    std::vector<dj::ContactP<T>> contacts; for (auto& c : s->M.contacts) contacts.push_back(dj::cast_contact<T>(c));
    if (contacts.empty()) contacts.push_back(dj::ContactP<T>());
    ENSURE(s->d_nodes, nodes.size() * sizeof(dj::NodeP<T>));
    ENSURE(s->d_contacts, contacts.size() * sizeof(dj::ContactP<T>));
    HIPCHK(hipMemcpy(s->d_nodes, nodes.data(), nodes.size() * sizeof(dj::NodeP<T>), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(s->d_contacts, contacts.data(), contacts.size() * sizeof(dj::ContactP<T>), hipMemcpyHostToDevice));
    if (s->M.has_tsd) {
        std::vector<dj::TraSD<T>> tsd;
        for (auto& a : s->M.tsd) { dj::TraSD<T> b; b.spring = T(a.spring); b.damper = T(a.damper); for (int i = 0; i < 3; ++i) b.off[i] = T(a.off[i]); b.lim_lo = T(a.lim_lo); b.lim_hi = T(a.lim_hi); b.nlim = a.nlim; tsd.push_back(b); }
        ENSURE(s->d_tsd, tsd.size() * sizeof(dj::TraSD<T>));
        HIPCHK(hipMemcpy(s->d_tsd, tsd.data(), tsd.size() * sizeof(dj::TraSD<T>), hipMemcpyHostToDevice));
    }
    if (s->M.has_cut) {
        std::vector<dj::NodeP<T>> cn; for (auto& n_ : s->M.cuts) cn.push_back(dj::cast_node<T>(n_));
        ENSURE(s->d_cuts, cn.size() * sizeof(dj::NodeP<T>));
        HIPCHK(hipMemcpy(s->d_cuts, cn.data(), cn.size() * sizeof(dj::NodeP<T>), hipMemcpyHostToDevice));
        ENSURE(s->d_cutws, (size_t)s->B * dj::CUTWS * sizeof(T));
    }
    if (s->M.has_mlim) {
        std::vector<dj::MLimP<T>> ml;
        for (auto& a : s->M.mlim) { dj::MLimP<T> b; b.nt = a.nt; b.nr = a.nr; for (int i = 0; i < 6; ++i) { b.lo[i] = T(a.lo[i]); b.hi[i] = T(a.hi[i]); } ml.push_back(b); }
        ENSURE(s->d_mlim, ml.size() * sizeof(dj::MLimP<T>));
        HIPCHK(hipMemcpy(s->d_mlim, ml.data(), ml.size() * sizeof(dj::MLimP<T>), hipMemcpyHostToDevice));
    }
    {   // the rows of the compact observation Jacobian that touch a body: those of its own joint (child half) and of every joint whose parent it is,
        // as entries 2 row + half in ascending order (the summation order of the closed-loop sweep's M^T go)
        const int Nb = s->M.Nb;
        std::vector<int> tp(Nb + 1, 0), te;
        for (int b = 0; b < Nb; ++b) {
            std::vector<int> e;
            for (int k = 0; k < Nb; ++k) {
                const auto& n_ = s->M.nodes[k];
                if (k != b && n_.parent != b) continue;
                for (int l = 0; l < 2 * (n_.nu_t + n_.nu_r); ++l) e.push_back(2 * (2 * n_.u_off + l) + (k == b ? 1 : 0));
            }
            std::sort(e.begin(), e.end());
            te.insert(te.end(), e.begin(), e.end()); tp[b + 1] = (int)te.size();
        }
        ENSURE(s->d_touch_ptr, tp.size() * sizeof(int)); ENSURE(s->d_touch_ent, (te.size() + 1) * sizeof(int));
        HIPCHK(hipMemcpy(s->d_touch_ptr, tp.data(), tp.size() * sizeof(int), hipMemcpyHostToDevice));
        if (!te.empty()) HIPCHK(hipMemcpy(s->d_touch_ent, te.data(), te.size() * sizeof(int), hipMemcpyHostToDevice));
    }
    std::vector<int> order;
    for (int lev = 0; lev <= s->M.maxlevel; ++lev) for (int b = 0; b < s->M.Nb; ++b) if (s->M.nodes[b].level == lev) order.push_back(b);
    ENSURE(s->d_order, order.size() * sizeof(int));
    HIPCHK(hipMemcpy(s->d_order, order.data(), order.size() * sizeof(int), hipMemcpyHostToDevice));
    return DOJO_OK;
}

int mapping_waves(const dj::HostModel& M);
bool quad_mapping_of(const DojoSim* s);
// wavefronts per workgroup of the quad mapping for this mechanism; 0 = lane mapping
int mapping_waves(const dj::HostModel& M) {
    // translational springs / dampers / limits: the quad builds that carry them are the single-wavefront ones with <= 4 contacts per body;
    // larger mechanisms take the lane mapping (its DJ_TSD builds: k_*_{4,8}_0_tsd)
    if (M.has_mlim || M.has_cut) return 0;                                // joint limits on several coordinates / both halves, kinematic loops: k_*_{4,8}_0_gen
    if (M.has_tsd && (M.S > 16 || M.maxc > 4)) return 0;
    if (M.contact_model == 2 && (M.S > 16 || M.maxc > 4)) return 0;       // LinearContact likewise (k_*_{4,8}_0_lin)
    if (M.S <= 16) return 1;
    if (M.S <= 32 && M.maxc <= 4 && M.Nc <= 16) return 2;
    return 0;
}

bool quad_mapping_of(const DojoSim* s) { return mapping_waves(s->M) > 0; }

int drain_slot(DojoSim* s, DojoSim::Ev3& e) {
    if (!e.used) return DOJO_OK;
    HIPCHK(hipEventSynchronize(e.b));
    float t = 0, t1 = 0;
    HIPCHK(hipEventElapsedTime(&t, e.a, e.b));
    if (e.has_mid) { HIPCHK(hipEventElapsedTime(&t1, e.a, e.m)); s->acc_step_ms += t1; s->acc_ift_ms += (double)t - t1; }
    else s->acc_step_ms += t;
    s->acc_n += e.n;
    e.used = false;
    return DOJO_OK;
}
int acquire_slot(DojoSim* s, int* idx) {
    if (s->ring.empty()) {
        s->ring.resize(64);
        for (auto& e : s->ring) { HIPCHK(hipEventCreate(&e.a)); HIPCHK(hipEventCreate(&e.m)); HIPCHK(hipEventCreate(&e.b)); }
    }
    *idx = (int)(s->ring_next++ % s->ring.size());
    return drain_slot(s, s->ring[*idx]);
}

// Environments are independent, so a batch is stepped as NG groups on internal streams: a group that contains an
// environment running into max_iter (one wavefront, ~5x the mean step time) delays only itself while the other groups'
// launches keep the GPU busy.  ROCm multiplexes HIP streams onto GPU_MAX_HW_QUEUES hardware queues (default 4) and
// streams that share a queue serialize, so the count stays below that.
// Refinement threshold: explicit (dojo_set_refinement) or tied to the requested tolerances -- the reference's defaults
// (rtol 1e-6, btol 1e-4) are met by the plain solves; tighter ones enable the refining kernels.
double refine_threshold(const DojoSim* s) {
    if (s->M.contact_model == 2) return (double)INFINITY;       // LinearContact builds carry no refining kernels
    if (s->M.has_ss) return (double)INFINITY;                   // ... nor do the body-body contact builds
    return s->refine_w >= 0.0 ? s->refine_w : ((s->opts.rtol <= 1e-7 || s->opts.btol <= 1e-6) ? DOJO_DEFAULT_REFINE_STIFFNESS : (double)INFINITY);
}
// scalars per contact in the exported [s; gamma] block: 8 (NonlinearContact; ImpactContact uses the first of each four), 12 (LinearContact)
size_t csg_per(const DojoSim* s) { return s->M.contact_model == 2 ? 12 : 8; }
// does the batch have more workgroups than the GPU holds at once (these kernels: one wavefront per SIMD, four SIMDs per compute unit)?
bool several_rounds(const DojoSim* s) {
    const int NW = mapping_waves(s->M);
    const size_t E = (size_t)std::max(1, 64 * (NW > 0 ? NW : 1) / (s->M.S * (NW > 0 ? 4 : 1)));
    return ((size_t)s->B + E - 1) / E * (size_t)std::max(NW, 1) > (size_t)4 * (size_t)(s->sm_count > 0 ? s->sm_count : 256);
}
size_t group_count(const DojoSim* s, bool want, bool joined_steps = false) {
    const size_t B = (size_t)s->B;
    size_t NG = (want && B >= 512) ? std::min<size_t>(16, B / 256) : 1;
    // An asynchronous handle (dojo_set_async) chains its groups' steps: a group that holds a long solve delays only itself, so below 4096 environments
    // smaller groups hide more of that tail than 256-environment ones -- down to 64 WORKGROUPS per group, for the single-wavefront quad mapping
    // (Ant, Quadruped: one environment per wavefront; the Block's sixteen per wavefront leave its B = 1024 at four groups: sixteen launches of
    // four wavefronts halved its rate).  profiles/r06_f_small_batches.txt: Ant B = 1024 0.47 -> 0.60 M, B = 2048 0.94 -> 1.02-1.09 M, B = 512
    // 0.30 -> 0.37 M; Quadruped B = 1024 0.48 -> 0.66 M.  The two-wavefront mapping keeps the 256-environment groups (Atlas B = 2048 with 16 groups:
    // +4 % on BASELINE's perturbation, -1 % standing, -19 % over the landing steps), and so does a handle that joins after every step: the groups'
    // launches are on its critical path.
    if (s->async && want && mapping_waves(s->M) == 1) {
        const size_t per_wg = std::max<size_t>(1, 16 / (size_t)std::max(1, s->M.S));      // environments per 64-lane workgroup (16 supernode slots)
        const size_t min_envs = 64 * per_wg;
        if (B >= 2 * min_envs) NG = std::max<size_t>(NG, std::min<size_t>(16, B / min_envs));
    }
    // A handle that joins after every step and whose batch takes several rounds of workgroups: two groups.  Each launch then has the whole GPU for
    // its rounds (with the dispatch order: its long solves first), and the IFT kernel of the first group runs under the tail of the second's step
    // kernel.  profiles/r06_i_dispatch.txt, joined ms per step at 1 / 2 / 4 / 8 / 16 groups: Ant B = 4096 5.93 / 5.84 / 6.19 / 6.14 / 6.28
    // (batch order: 6.45 / 6.22 / 6.47 / 6.48 / 6.49), Atlas B = 2048 6.57 / 6.35 / 6.70 / 6.89 / 6.85, Quadruped B = 8192 12.5 / 12.1 / 12.1 / 12.0 / 11.9.
    if (joined_steps && !s->async && want && several_rounds(s)) NG = std::min<size_t>(NG, 2);
    if (s->groups > 0) NG = std::min<size_t>(std::min<size_t>((size_t)s->groups, 16), std::max<size_t>(1, B / 64));   // (more than 16 queues in flight collapse: 0.68 M against 1.00 M at 24, same session)
    const char* hq = getenv("GPU_MAX_HW_QUEUES");
    const int nq = hq ? atoi(hq) : 4;
    NG = std::min<size_t>(NG, (size_t)std::max(1, nq - 1));
    // The refining kernels keep 2-6 KB of scratch per lane, and ROCr sizes a hardware queue's scratch for a full GPU of such
    // wavefronts (~3 GB): sixteen queues asking for it at once end in HSA_STATUS_ERROR_OUT_OF_RESOURCES (the queue aborts the
    // process).  With refinement in force the batch is stepped as at most three groups (seen green; the default queue count).
    if (std::isfinite(refine_threshold(s))) NG = std::min<size_t>(NG, 3);
    // The general lane-mapping builds (several limits per joint, cut elements) keep ~40 KB of scratch per lane (the small dense system of the cut
    // elements, the per-coordinate limit rows): one queue's worth of it at a time
    if (s->M.has_mlim || s->M.has_cut) NG = 1;
    return NG;
}
int ensure_groups(DojoSim* s, size_t NG) {
    while (s->gstreams.size() < NG) {
        hipStream_t g_; HIPCHK(hipStreamCreateWithFlags(&g_, hipStreamNonBlocking)); s->gstreams.push_back(g_);
        hipEvent_t gev_; HIPCHK(hipEventCreateWithFlags(&gev_, hipEventDisableTiming)); s->gevents.push_back(gev_);
    }
    if (!s->fork_event) HIPCHK(hipEventCreateWithFlags(&s->fork_event, hipEventDisableTiming));
    return DOJO_OK;
}
// pipelined groups (dojo_set_async(h, 2)): a second stream per group for its IFT kernels, events, the second hand-off record
// (the IFT streams are shared: ROCm runs ~20 streams side by side before the hardware queues are time-sliced -- 24 collapse --, so the 16 groups get
//  pipe_streams() of them, group g on stream g % n; the IFT kernels of the groups that share one run one after the other, off the critical path)
size_t pipe_streams() { static const char* e_ = getenv("DOJO_PIPE_STREAMS"); const int n = e_ ? atoi(e_) : 4; return (size_t)std::max(1, std::min(n, 16)); }
int ensure_pipe(DojoSim* s, size_t NG) {
    while (s->gstreams2.size() < std::min(NG, pipe_streams())) {
        hipStream_t g_; HIPCHK(hipStreamCreateWithFlags(&g_, hipStreamNonBlocking)); s->gstreams2.push_back(g_);
        hipEvent_t jev_; HIPCHK(hipEventCreateWithFlags(&jev_, hipEventDisableTiming)); s->gevents2.push_back(jev_);
    }
    while (s->grad_done[0].size() < NG)
        for (int p = 0; p < 2; ++p) { hipEvent_t dev_; HIPCHK(hipEventCreateWithFlags(&dev_, hipEventDisableTiming)); s->grad_done[p].push_back(dev_); }
    while (s->main_events.size() < NG) { hipEvent_t ev_; HIPCHK(hipEventCreateWithFlags(&ev_, hipEventDisableTiming)); s->main_events.push_back(ev_); }
    ENSURE(s->d_sol2, (size_t)s->B * s->M.S * dj::HANDOFF_MAX * sizeof(double));
    return DOJO_OK;
}
// the caller's stream waits for everything the environment groups have in flight
int join_groups(DojoSim* s, hipStream_t st) {
    if (!s->pending) return DOJO_OK;
    for (size_t gi = 0; gi < s->gstreams.size(); ++gi) { HIPCHK(hipEventRecord(s->gevents[gi], s->gstreams[gi])); HIPCHK(hipStreamWaitEvent(st, s->gevents[gi], 0)); }
    for (size_t gi = 0; gi < s->gstreams2.size(); ++gi) { HIPCHK(hipEventRecord(s->gevents2[gi], s->gstreams2[gi])); HIPCHK(hipStreamWaitEvent(st, s->gevents2[gi], 0)); }
    s->pending = false;
    return DOJO_OK;
}

// the iteration cap in force for this handle's next step, 0 = none: the continuation kernel exists for the single-wavefront quad mapping
// (<= 16 bodies) with plain solves (no refinement), NonlinearContact / no contacts (the variants that carry an IFT)
int effective_cap(const DojoSim* s) {
    static const char* ecap_ = getenv("DOJO_ITER_CAP");
    const int cap = s->iter_cap >= 0 ? s->iter_cap : (ecap_ ? atoi(ecap_) : DOJO_DEFAULT_ITERATION_CAP);
    if (cap <= 0 || cap >= s->opts.max_iter) return 0;
    if (mapping_waves(s->M) != 1 || std::isfinite(refine_threshold(s))) return 0;
    if (s->M.contact_model != 0 || s->M.has_ss) return 0;
    return cap;
}
// what a capped step needs besides the groups' streams: the continuation's stream, its end event, a "step kernel done" event per group,
// the list and its count (zeroed here, on `st`, before the step kernels are forked off it)
int begin_capped_step(DojoSim* s, size_t NG, hipStream_t st) {
    if (!s->cstream) {
        // (DOJO_CONT_PRIORITY=1: a high-priority stream.  Measured: with it the step kernels of the FOLLOWING step take 20..300 ms on some
        //  queues -- the scheduler's handling of queue priorities, presumably wave save / restore -- so the default is a plain stream, and
        //  the order of submission below is what puts the continuation in front of the IFT kernels)
        static const bool prio_ = getenv("DOJO_CONT_PRIORITY") != nullptr && atoi(getenv("DOJO_CONT_PRIORITY")) != 0;
        int lo_ = 0, hi_ = 0; HIPCHK(hipDeviceGetStreamPriorityRange(&lo_, &hi_));
        if (prio_) HIPCHK(hipStreamCreateWithPriority(&s->cstream, hipStreamNonBlocking, hi_));
        else HIPCHK(hipStreamCreateWithFlags(&s->cstream, hipStreamNonBlocking));
    }
    if (!s->allmain_event) HIPCHK(hipEventCreateWithFlags(&s->allmain_event, hipEventDisableTiming));
    if (!s->cont_event) HIPCHK(hipEventCreateWithFlags(&s->cont_event, hipEventDisableTiming));
    while (s->main_events.size() < NG) { hipEvent_t ev_; HIPCHK(hipEventCreateWithFlags(&ev_, hipEventDisableTiming)); s->main_events.push_back(ev_); }
    const int NW = mapping_waves(s->M), E = 64 * NW / (s->M.S * 4);
    ENSURE(s->d_cont_list, (((size_t)s->B + E - 1) / E + 1) * sizeof(int)); ENSURE(s->d_cont_count, sizeof(int));
    HIPCHK(hipMemsetAsync(s->d_cont_count, 0, sizeof(int), st));
    return DOJO_OK;
}

// One step launch, by job: refusals, the kernel build, workspaces, kernel arguments, timing, the kernels behind the step.  First what the kernels do not
// compute: it depends on the handle and on what is asked for (dz / du, or dc), not on the environments of a launch -- an entry point asks once, before it enqueues anything.
int refuse_unsupported(const DojoSim* s, bool want_dz, bool want_dc) {
    const size_t Nb = s->M.Nb, nu = s->M.nu;
    const bool g = want_dz || want_dc, quad = quad_mapping_of(s);
    if (g && (s->M.has_ss || s->M.has_cc)) { g_err = "gradients are not available for mechanisms with a body-body contact"; return DOJO_ERR_UNSUPPORTED; }
    if (g && s->M.contact_model != 0) {   // the reference has no data Jacobians for ImpactContact / LinearContact either (src/gradients/data.jl:152-192 are NonlinearContact methods)
        g_err = "gradients are not available for ImpactContact / LinearContact mechanisms"; return DOJO_ERR_UNSUPPORTED;
    }
    if (g && quad && std::max<size_t>(2 * Nb + (nu + 5) / 6, want_dc ? (size_t)s->M.Nc : 0) > 128) {
        // (dojo_device.hpp, gradient_columns_quad: the branch schedule keeps batch sets in two 64-bit words; unreachable with <= 32 bodies -- 2 x 32 + 32 --
        //  but a mapping change must not turn it into silently aliased batches)
        g_err = "the IFT sweeps support at most 128 column batches per environment"; return DOJO_ERR_UNSUPPORTED;
    }
    if (want_dc && s->M.Nc > 64) {  // the sweeps' batch masks hold one bit per contact of the environment (dojo_device.hpp, sweep_masks)
        g_err = "contact-data gradients support at most 64 contacts per environment"; return DOJO_ERR_UNSUPPORTED;
    }
    if (want_dc && !quad) { g_err = "contact-data gradients need the quad mapping (<= 32 bodies)"; return DOJO_ERR_UNSUPPORTED; }
    return DOJO_OK;
}

// The kernel builds (one object file of dojo_kernels.hip each): family x contacts-per-body bound (MAXC) x mapping (wavefronts per workgroup of the quad
// mapping, 0 = lane mapping), the launchers of both ABI types as [f64, f32].  sol_rec: doubles per supernode of the build's step -> IFT hand-off record.
typedef int (*launcher_t)(const void*, int, void*, int, void*); typedef int (*claunch_t)(const void*, int, void*);
enum { FAM_PLAIN, FAM_TSD, FAM_GEN, FAM_LIN, FAM_SS };
struct Variant { int family, maxc, waves; launcher_t step[2]; claunch_t cgrad[2]; size_t sol_rec; };
#define DJ_V(fam, pre, mc, nw) {fam, mc, nw, {dojo_launch_##pre##double_##mc##_##nw, dojo_launch_##pre##float_##mc##_##nw}, {nullptr, nullptr}, (size_t)dj::HandOff<mc, fam == FAM_GEN>::size}
#define DJ_VC(fam, pre, mc, nw) {fam, mc, nw, {dojo_launch_##pre##double_##mc##_##nw, dojo_launch_##pre##float_##mc##_##nw}, \
                                 {dojo_launch_cgrad_##pre##double_##mc##_##nw, dojo_launch_cgrad_##pre##float_##mc##_##nw}, (size_t)dj::HandOff<mc, false>::size}
const Variant g_variants[] = {        // (rows of one family and mapping: MAXC ascending)
    DJ_VC(FAM_PLAIN, , 1, 1), DJ_VC(FAM_PLAIN, , 4, 1), DJ_VC(FAM_PLAIN, , 8, 1), DJ_VC(FAM_PLAIN, , 1, 2), DJ_VC(FAM_PLAIN, , 4, 2), DJ_V(FAM_PLAIN, , 4, 0), DJ_V(FAM_PLAIN, , 8, 0),
    DJ_VC(FAM_TSD, tsd_, 1, 1), DJ_VC(FAM_TSD, tsd_, 4, 1), DJ_V(FAM_TSD, tsd_, 4, 0), DJ_V(FAM_TSD, tsd_, 8, 0),
    DJ_V(FAM_GEN, gen_, 4, 0), DJ_V(FAM_GEN, gen_, 8, 0),
    DJ_V(FAM_LIN, lin_, 1, 1), DJ_V(FAM_LIN, lin_, 4, 1), DJ_V(FAM_LIN, lin_, 4, 0), DJ_V(FAM_LIN, lin_, 8, 0),
    DJ_V(FAM_SS, ss_, 1, 1)};
// the build that serves a mechanism under the mapping NW (mapping_waves): of its family and mapping, the smallest MAXC that holds its contacts per body
// (the largest where none does); null: no such build
const Variant* variant_of(const dj::HostModel& M, int NW) {
    const int fam = (M.has_ss && M.contact_model != 2) ? FAM_SS : M.contact_model == 2 ? FAM_LIN : (M.has_mlim || M.has_cut) ? FAM_GEN : M.has_tsd ? FAM_TSD : FAM_PLAIN;
    const Variant* v = nullptr;
    for (const Variant& r : g_variants) if (r.family == fam && r.waves == NW && (!v || v->maxc < M.maxc)) v = &r;
    return v;
}

// How a span maps onto workgroups.  Four lanes per supernode when the mechanism has <= 16 bodies (one Ant per wavefront) or <= 32 bodies (one Atlas per
// two-wavefront workgroup; contact rows pooled per contact: <= 16 contacts, <= 4 per body); else one lane per supernode.
struct Geometry {
    int NW; bool quad; int E; size_t lanes;     // wavefronts per workgroup (0: lane mapping); environments and lanes per workgroup
    size_t grid, waves_total, wave0;            // workgroups of the span, of the batch, in front of the span
    long long ypark_stride, msg_stride;         // elements per workgroup / per environment of the IFT's parking and message buffers (0: not used)
};
Geometry geometry_of(const DojoSim* s, const Span& sp, bool g) {
    const int NW = mapping_waves(s->M), E = 64 * (NW > 0 ? NW : 1) / (s->M.S * (NW > 0 ? 4 : 1));
    Geometry ge{NW, NW > 0, E, (size_t)64 * NW, (size_t)(sp.nenv + E - 1) / E, ((size_t)s->B + E - 1) / E, sp.env0 / E, 0, 0};
    if (g && ge.quad) {                         // (dojo_device.hpp, gradient_columns_quad)
        const size_t batches = std::max<size_t>(2 * s->M.Nb + (s->M.nu + 5) / 6, (size_t)s->M.Nc);     // state + control batches | contact batches (dojo_cgrad_kernel)
        if (s->w < sizeof(double)) ge.ypark_stride = (long long)(batches * 18 * ge.lanes);      // fp32 ABI: all four roles park (LU-form sweeps)
        size_t ntops = 0; for (auto& n_ : s->M.nodes) if (n_.level <= 1) ++ntops;      // one block per level-1 supernode (messages) and per root (its Δv, Δω)
        ge.msg_stride = (long long)(ntops * batches * 36 + 8);      // what the children of a root post to its body rows (+ a trash slot for the stores of columns that do not exist)
    }
    return ge;
}

// the handle's workspaces a launch uses, allocated on first use (all in the arithmetic type of the kernels, fp64)
int ensure_workspaces(DojoSim* s, const StepIO& io, const Mode& m, const Geometry& ge, bool g, bool reorder) {
    const size_t B = s->B, wT = sizeof(double), sol_bytes = B * s->M.S * dj::HANDOFF_MAX * wT;       // (the hand-off: sized for the largest record)
    if (g) {
        ENSURE(s->d_sol, sol_bytes);
        if (ge.quad) { ENSURE(s->d_fac, ge.waves_total * dj::FAC_PER_LANE * ge.lanes * wT); ENSURE(s->d_lu, ge.waves_total * dj::LU_PER_LANE * ge.lanes * wT); }
        if (ge.ypark_stride) ENSURE(s->d_ypark, ge.waves_total * (size_t)ge.ypark_stride * wT);
        if (ge.msg_stride) ENSURE(s->d_msg, B * (size_t)ge.msg_stride * wT);
    }
    if (m.phase != PH_ALL) { ENSURE(s->d_sol, sol_bytes); ENSURE(s->d_resume, B * dj::CARRY_PER_ENV * wT); if (!io.status) ENSURE(s->d_cstat, B * sizeof(int)); }
    if (reorder) { ENSURE(s->d_dispatch, (ge.waves_total + 1) * sizeof(int)); if (!io.iters) ENSURE(s->d_liters, B * sizeof(int)); }
    // the refining kernels follow the plain ones (dojo_kernels.hip)
    if (ge.quad && std::isfinite(refine_threshold(s))) { ENSURE(s->d_blk, ge.waves_total * 90 * ge.lanes * wT); ENSURE(s->d_flag, B * sizeof(int)); }
    return DOJO_OK;
}

// the arguments of the kernels of one launch: the batch-level buffers moved to the span's first environment / workgroup
template <class TIO, class T>
dj::KernelArgs<TIO, T> kernel_args(const DojoSim* s, const StepIO& io, const Span& sp, const Mode& m, const Geometry& ge, const Variant& v, bool reorder) {
    const size_t Nb = s->M.Nb, nu = s->M.nu, nx = 12 * Nb, env0 = sp.env0, wave0 = ge.wave0;
    const bool g = io.dz != nullptr || io.dc != nullptr, quad = ge.quad, step = io.dc == nullptr;      // (contact-data columns only: the step's solution is not written again)
    auto off = [&](const void* p, size_t per_env) -> TIO* { return p ? (TIO*)p + env0 * per_env : (TIO*)nullptr; };
    dj::KernelArgs<TIO, T> A;
    A.G = dj::make_globals<T>(s->M, s->opts, s->grad_mode, refine_threshold(s));
    if (ge.NW == 1 || ge.NW == 2) dj::set_row_passes(A.G, s->M);             // the factorization's level passes in the row layout (dojo_device.hpp, factorize_rows), where they pay
    A.nodes = (const dj::NodeP<T>*)s->d_nodes; A.contacts = (const dj::ContactP<T>*)s->d_contacts; A.B = sp.nenv;
    A.z = off(io.z, 13 * Nb); A.u = off(io.u, nu); A.z_next = off(io.z_next, 13 * Nb); A.fext = off(s->fext, 6 * Nb);
    A.status = io.status ? io.status + env0 : nullptr; A.iters = io.iters ? io.iters + env0 : nullptr;
    A.vel = off(step ? s->d_vel : nullptr, 6 * Nb); A.joint_imp = off(step ? s->d_jimp : nullptr, s->M.n_joint_imp); A.contact_sg = off(step ? s->d_csg : nullptr, csg_per(s) * s->M.Nc);
    A.dz = off(io.dz, nx * nx); A.du = off(io.du, nx * nu); A.dc = off(io.dc, nx * 5 * s->M.Nc);
    A.res = io.storage ? off(s->d_res, 6 * Nb) : (TIO*)nullptr;
    A.tsd = s->M.has_tsd ? (const dj::TraSD<T>*)s->d_tsd : nullptr;
    A.mlim = s->M.has_mlim ? (const dj::MLimP<T>*)s->d_mlim : nullptr;
    A.cuts = s->M.has_cut ? (const dj::NodeP<T>*)s->d_cuts : nullptr; A.ncut = (int)s->M.cuts.size();
    A.cutws = s->M.has_cut ? (T*)s->d_cutws + env0 * (size_t)dj::CUTWS : nullptr;
    A.mu_out = s->d_mu ? (T*)s->d_mu + env0 : nullptr;
    A.diag_out = (s->d_diag && quad) ? (T*)s->d_diag + 2 * env0 : nullptr;
    // (the record size of the kernels of this mechanism: a launch over the whole batch -- the continuation -- must find the records where the groups' launches put them)
    A.sol = (g || m.phase != PH_ALL) ? (T*)(m.rec ? s->d_sol2 : s->d_sol) + env0 * s->M.S * v.sol_rec : nullptr;
    // the explicit inverses of the Newton loop travel only when somebody reads them: the refining IFT kernel
    A.fac = (g && quad && A.G.refine_w < INFINITY) ? (T*)s->d_fac + wave0 * dj::FAC_PER_LANE * ge.lanes : nullptr;
    A.lu = (g && quad) ? (T*)s->d_lu + wave0 * dj::LU_PER_LANE * ge.lanes : nullptr;
    A.ypark_stride = ge.ypark_stride; A.ypark = ge.ypark_stride ? (T*)s->d_ypark + wave0 * (size_t)ge.ypark_stride : nullptr;
    A.msg_stride = ge.msg_stride; A.msg = ge.msg_stride ? (T*)s->d_msg + env0 * (size_t)ge.msg_stride : nullptr;
    // Iteration cap (phased launches only; dojo_step_dev has checked that it applies and has zeroed the list's count): the solves that are
    // unfinished after `cap` Newton iterations leave the step kernel and go on in the continuation kernel (PH_CONT)
    A.G.iter_cap = 0;
    if (m.phase != PH_ALL) {
        if (m.cap_lists) {
            A.G.iter_cap = effective_cap(s);
            A.resume = (T*)s->d_resume + env0 * dj::CARRY_PER_ENV;
            A.cont_list = s->d_cont_list; A.cont_count = s->d_cont_count; A.wave_base = (int)wave0;
        }
        if (!io.status) A.status = s->d_cstat + env0;
    }
    // Dispatch order: this launch's step kernel hands its workgroups out by the permutation the previous launch over the same environments left behind
    if (reorder) {
        if (!A.iters) A.iters = s->d_liters + env0;
        auto it_ = s->dispatch_have.find(wave0);
        if (it_ != s->dispatch_have.end() && it_->second == sp.nenv) A.dispatch = s->d_dispatch + wave0;
    }
    A.blk = nullptr; A.flag = nullptr;
    if (quad && A.G.refine_w < INFINITY) { A.blk = (T*)s->d_blk + wave0 * 90 * ge.lanes; A.flag = s->d_flag + env0; }
    return A;
}

// Timed launches: a slot of the ring, its begin event in front of the first kernel ...
int begin_timing(DojoSim* s, int* slot, hipStream_t st) {
    TRY(acquire_slot(s, slot)); HIPCHK(hipEventRecord(s->ring[*slot].a, st));
    return DOJO_OK;
}
// ... and its end event behind the last one; the slot then stands for n steps (has_mid: the launcher put the slot's middle event between step and IFT kernel)
int end_timing(DojoSim* s, int slot, bool has_mid, int n, hipStream_t st) {
    DojoSim::Ev3& e = s->ring[slot]; HIPCHK(hipEventRecord(e.b, st));
    e.has_mid = has_mid; e.n = n; e.used = true; s->last_slot = slot;
    return DOJO_OK;
}

// Dispatch order, behind a launch's kernels: the permutation for the next launch over these environments, from this step's iteration counts
int launch_dispatch_order(DojoSim* s, const int* iters, const Span& sp, const Geometry& ge) {
    // (segments of another partition of the batch that overlap this one hold permutations of other ranges: forgotten before this one is written)
    for (auto it_ = s->dispatch_have.begin(); it_ != s->dispatch_have.end();) {
        const size_t a_ = it_->first, b_ = a_ + ((size_t)it_->second + ge.E - 1) / ge.E;
        if (a_ < ge.wave0 + ge.grid && ge.wave0 < b_) it_ = s->dispatch_have.erase(it_); else ++it_;
    }
    hipLaunchKernelGGL(dispatch_order_kernel, dim3(1), dim3(1024), 0, sp.stream, iters, sp.nenv, ge.E, (int)ge.grid, s->d_dispatch + ge.wave0);
    HIPCHK(hipGetLastError());
    s->dispatch_have[ge.wave0] = sp.nenv;
    return DOJO_OK;
}
// The kernels of dojo_coord_kernels.hpp, one launcher each: the grid, the casts and the launch check are here, once for both ABI types.
// One thread per item, T_ threads per workgroup:
template <class K, class... Args>
int launch_items(K kernel, long long items, int T_, hipStream_t st, Args... args) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)((items + T_ - 1) / T_)), dim3(T_), 0, st, args...);
    HIPCHK(hipGetLastError());
    return DOJO_OK;
}
const dj::NodeP<double>* node_table(const DojoSim* s) { return (const dj::NodeP<double>*)s->d_nodes; }
// record: the Storage rows of the environments of a launch, one thread per (environment, body)
template <class TIO>
int launch_storage(const DojoSim* s, const StepIO& io, const Span& sp) {
    return launch_items(dj::ckern::storage_kernel<TIO>, (long long)sp.nenv * s->M.Nb, 128, sp.stream, node_table(s), (const dj::ContactP<double>*)s->d_contacts, s->M.Nb, s->M.Nc,
                        s->M.contact_model, (int)csg_per(s), s->M.dt, (int)sp.env0, sp.nenv, (const TIO*)io.z, (const TIO*)s->d_vel, (const TIO*)s->d_csg, (const TIO*)s->d_res,
                        (const TIO*)s->fext, (TIO*)io.storage);
}
// ... the others over the whole batch, device arrays in:
template <class TIO> int launch_min2max(const DojoSim* s, const void* x, void* z, hipStream_t st) {      // one thread per environment
    return launch_items(dj::ckern::min2max_kernel<TIO>, s->B, 64, st, node_table(s), (const int*)s->d_order, s->M.Nb, (int)s->M.nu, s->M.dt, s->B, (const TIO*)x, (TIO*)z);
}
template <class TIO> int launch_max2min(const DojoSim* s, const void* z, void* x, int ldx, hipStream_t st) {      // per (environment, joint); ldx: scalars per row of x
    return launch_items(dj::ckern::max2min_kernel<TIO>, (long long)s->B * s->M.Nb, 256, st, node_table(s), s->M.Nb, (int)s->M.nu, s->M.dt, s->B, (const TIO*)z, (TIO*)x, ldx);
}
template <class TIO> int launch_contact_obs(const DojoSim* s, void* obs, int ldx, hipStream_t st) {      // per (environment, contact), behind the 2 nu minimal coordinates of a row
    return launch_items(dj::ckern::contact_obs_kernel<TIO>, (long long)s->B * s->M.Nc, 256, st, s->M.Nc, s->B, (const TIO*)s->d_csg, (TIO*)obs, ldx, 2 * (int)s->M.nu);
}
template <class TIO> int launch_next_state(const DojoSim* s, const void* z, void* z_out, hipStream_t st) {      // per (environment, body)
    return launch_items(dj::ckern::next_state_kernel<TIO>, (long long)s->B * s->M.Nb, 256, st, s->M.Nb, s->M.dt, s->B, (const TIO*)z, (TIO*)z_out);
}
template <class TIO> int launch_fold_impulses(const DojoSim* s, const void* jf, void* out, hipStream_t st) {      // per scalar of [B][6Nb]: the handle's external force + jf / dt
    const long long n = (long long)s->B * 6 * s->M.Nb;
    return launch_items(dj::ckern::fold_impulses_kernel<TIO>, n, 256, st, n, (const TIO*)s->fext, (const TIO*)jf, 1.0 / s->M.dt, (TIO*)out);
}
// the chain of get_minimal_gradients! over the handle's d_dz, d_du: the min -> max Jacobian at (x, z) into d_jm, the max -> min blocks at d_zn (advanced by a step with
// `advance`) into d_jb, d_jt = dz d_jm, and jx, ju = blocks * (d_jt, du).  The two Jacobian kernels per environment / per (environment, joint), the products one workgroup per environment.
// For the environments of `sp` on its stream: all pointers are batch-level, the kernels index from 0 and are given the span's slice of each (the workspaces are batch-sized, so
// the groups of a rollout own disjoint slices of them).
template <class TIO> int launch_minimal_chain(const DojoSim* s, const Span& sp, const void* x, const void* z, int advance, void* jx, void* ju) {
    const int B = sp.nenv, Nb = s->M.Nb, nu = (int)s->M.nu, T_ = 256;
    const size_t e0 = sp.env0, nx = 12 * (size_t)Nb, nm = 2 * (size_t)nu;
    hipStream_t st = sp.stream;
    double *jm = (double*)s->d_jm + e0 * nx * nm, *jt = (double*)s->d_jt + e0 * nx * nm, *jb = (double*)s->d_jb + e0 * Nb * 12 * 24;
    const TIO *xs = (const TIO*)x + e0 * nm, *zs = (const TIO*)z + e0 * 13 * Nb, *zn = (const TIO*)s->d_zn + e0 * 13 * Nb;
    const TIO *dz = (const TIO*)s->d_dz + e0 * nx * nx, *du = (const TIO*)s->d_du + e0 * nx * nu;
    TRY(launch_items(dj::ckern::min2max_jac_kernel<TIO>, B, 64, st, node_table(s), (const int*)s->d_order, Nb, nu, s->M.dt, B, xs, zs, jm));
    TRY(launch_items(dj::ckern::max2min_jac_kernel<TIO>, (long long)B * Nb, T_, st, node_table(s), Nb, s->M.dt, B, zn, advance, jb));
    TRY(launch_items(dj::ckern::chain_mid_kernel<TIO>, (long long)B * T_, T_, st, 12 * Nb, 2 * nu, B, dz, (const double*)jm, jt));
    return launch_items(dj::ckern::chain_out_kernel<TIO>, (long long)B * T_, T_, st, node_table(s), Nb, nu, B, (const double*)jb, (const double*)jt, du,
                        (TIO*)jx + e0 * nm * nm, ju ? (TIO*)ju + e0 * nm * nu : nullptr);
}

// Launches the step (and IFT) kernels for the environments of `sp`; all pointers of `io` are the batch-level buffers.
template <class TIO, class T, class TL>
int launch(DojoSim* s, const StepIO& io, const Span& sp, const Mode& m) {
    const hipStream_t st = sp.stream;
    const bool g = io.dz != nullptr || io.dc != nullptr, f32 = sizeof(TIO) == 4, timed = m.slot != nullptr && m.phase != PH_CONT;
    const Geometry ge = geometry_of(s, sp, g);
    const Variant* v = variant_of(s->M, ge.NW);
    if (!v || (io.dc && !v->cgrad[f32])) { g_err = "no kernel build serves this mechanism"; return DOJO_ERR_UNSUPPORTED; }
    // Dispatch order (dojo_set_dispatch_order): the permutation for the next launch is made behind this launch's kernels.
    // (mode 1: the order only matters when the GPU cannot hold the batch's workgroups at once)
    // (... and its launches are not chained next to other groups' -- an asynchronous handle of several groups, a rollout: a single launch per step
    //  waits for its last wavefront on an asynchronous handle too)
    const bool reorder = m.phase == PH_ALL && io.dc == nullptr && s->dispatch_mode != 0
                         && (s->dispatch_mode == 2 || ((!s->async || m.groups <= 1) && !m.chained && several_rounds(s)));
    TRY(ensure_workspaces(s, io, m, ge, g, reorder));
    const dj::KernelArgs<TIO, T> A = kernel_args<TIO, T>(s, io, sp, m, ge, *v, reorder);
    if (timed && m.phase != PH_GRAD) TRY(begin_timing(s, m.slot, st));      // (PH_GRAD: the slot of the group's PH_MAIN)
    // Test hook (tests/conftest.py sets it for the GPU tier): the Jacobian buffers are filled with NaN bit patterns before the IFT kernels run, so that
    // an entry the device fails to write comes back as NaN instead of whatever the allocation held (the kernels must write every entry).
    static const bool poison_ = getenv("DOJO_POISON_OUTPUTS") != nullptr;
    if (poison_ && g && (m.phase == PH_ALL || m.phase == (m.cap_lists ? PH_MAIN : PH_GRAD))) {    // (pipelined: on the IFT's stream, behind the previous step's IFT)
        const size_t nx = 12 * s->M.Nb, nu = s->M.nu, n = (size_t)sp.nenv;
        if (A.dc) HIPCHK(hipMemsetAsync(A.dc, 0xFF, n * nx * 5 * s->M.Nc * sizeof(TIO), st));
        if (!A.dc && A.dz) HIPCHK(hipMemsetAsync(A.dz, 0xFF, n * nx * nx * sizeof(TIO), st));
        if (!A.dc && A.du && nu > 0) HIPCHK(hipMemsetAsync(A.du, 0xFF, n * nx * nu * sizeof(TIO), st));
    }
    const int phases = m.phase == PH_ALL ? (1 | (g ? 2 : 0)) : m.phase == PH_MAIN ? 1 : m.phase == PH_GRAD ? 2 : (4 | (g ? 8 : 0));
    const int lgrid = m.phase == PH_CONT ? (int)std::min<size_t>(ge.waves_total, 128) : (int)ge.grid;     // (a continuation workgroup takes a whole CU's LDS and loops over the list)
    const int lrc = io.dc ? v->cgrad[f32](&A, (int)ge.grid, (void*)st)      // contact-data columns only: the hand-off of the last differentiable step is re-used
                          : v->step[f32](&A, lgrid, (void*)st, phases, (timed && g && (phases & 1)) ? (void*)s->ring[*m.slot].m : nullptr);
    if (lrc != 0) { g_err = std::string("kernel launch: ") + hipGetErrorString((hipError_t)lrc); return DOJO_ERR_DEVICE; }
    HIPCHK(hipGetLastError());
    if (timed && (m.phase == PH_ALL || m.phase == PH_GRAD || (m.phase == PH_MAIN && !g))) TRY(end_timing(s, *m.slot, g && !io.dc, 1, st));
    if (reorder) TRY(launch_dispatch_order(s, A.iters, sp, ge));
    if (io.storage) TRY(launch_storage<TIO>(s, io, sp));
    return DOJO_OK;
}

int launch_any(DojoSim* s, const StepIO& io, const Span& sp, const Mode& m) {
    return by_dtype(s, [&](auto t) { return launch<decltype(t), double, double>(s, io, sp, m); });
}
Mode step_mode(const DojoSim* s, size_t NG, bool cap_lists = false, bool chained = false) { return Mode{PH_ALL, nullptr, cap_lists, chained, NG, s->sol_cur}; }
Span whole_batch(const DojoSim* s, hipStream_t st) { return Span{0, s->B, st}; }

// A failure after the fork: what is already running on the internal streams must be ordered before the caller's stream all the same.  Armed where a step forks off the caller's
// stream; every return that does not go through done() marks the handle pending and joins the groups' streams -- and the continuation's, once its end event is recorded -- into it.
struct ForkGuard {
    DojoSim* s; hipStream_t st; bool armed = true, cont_recorded = false;
    ~ForkGuard() { if (!armed) return; s->pending = true; (void)join_groups(s, st); if (cont_recorded) (void)hipStreamWaitEvent(st, s->cont_event, 0); }
    int done() { armed = false; return DOJO_OK; }
};

// The three ways dojo_step_dev steps a batch, each its stream choreography.  One launch on the caller's stream:
int step_single(DojoSim* s, const StepIO& io, hipStream_t st, bool capped) {
    int slot = -1; TRY(join_groups(s, st));
    const Mode m = step_mode(s, 1, capped);
    if (!capped) return launch_any(s, io, whole_batch(s, st), m.with(PH_ALL, &slot));
    // (the continuation is enqueued before the IFT of the finished workgroups and on a stream of higher priority: its workgroups need a
    //  whole CU's LDS each, which they only find before the IFT's wavefronts have spread over the GPU)
    TRY(launch_any(s, io, whole_batch(s, st), m.with(PH_MAIN, &slot)));
    ForkGuard guard{s, st};
    HIPCHK(hipEventRecord(s->main_events[0], st));
    HIPCHK(hipStreamWaitEvent(s->cstream, s->main_events[0], 0));
    TRY(launch_any(s, io, whole_batch(s, s->cstream), m.with(PH_CONT, nullptr)));
    HIPCHK(hipEventRecord(s->cont_event, s->cstream)); guard.cont_recorded = true;
    if (io.dz) TRY(launch_any(s, io, whole_batch(s, st), m.with(PH_GRAD, &slot)));
    HIPCHK(hipStreamWaitEvent(st, s->cont_event, 0));
    return guard.done();
}

// fork: the step kernel of every group, each followed by the IFT of what it finished; behind ALL step kernels the continuation, once
// over the batch, on its own stream; join: the groups and the continuation into the caller's stream
int step_capped_groups(DojoSim* s, const StepIO& io, hipStream_t st, size_t NG) {
    TRY(ensure_groups(s, NG));
    const Partition P(s->B, NG); s->last_part = P;
    if (s->group_slot.size() < NG) s->group_slot.resize(NG, -1);
    const Mode m = step_mode(s, NG, true);
    ForkGuard guard{s, st};
    HIPCHK(hipEventRecord(s->fork_event, st));
    for (size_t gi = 0; gi < P.groups(); ++gi) {
        const Span sp = P.span(gi, s->gstreams[gi]);
        HIPCHK(hipStreamWaitEvent(sp.stream, s->fork_event, 0));
        TRY(launch_any(s, io, sp, m.with(PH_MAIN, &s->group_slot[gi])));
        HIPCHK(hipEventRecord(s->main_events[gi], sp.stream));
        HIPCHK(hipStreamWaitEvent(s->cstream, s->main_events[gi], 0));
    }
    // The continuation first: its workgroups take a whole CU's LDS each, which they only find while the GPU is empty -- so the groups' IFT
    // kernels wait until every step kernel is done as well (they would otherwise start behind their own group's step kernel, fill the CUs as
    // these drain, and keep the continuation out until they are through: measured, +1.2 ms per step), and the continuation's stream has
    // the higher priority.  The IFT kernels (1.2 ms of work) then run next to the continuation (2-3 ms on a few CUs).
    HIPCHK(hipEventRecord(s->allmain_event, s->cstream));
    TRY(launch_any(s, io, whole_batch(s, s->cstream), m.with(PH_CONT, nullptr)));
    HIPCHK(hipEventRecord(s->cont_event, s->cstream)); guard.cont_recorded = true;
    for (size_t gi = 0; gi < P.groups() && io.dz; ++gi) {
        const Span sp = P.span(gi, s->gstreams[gi]);
        HIPCHK(hipStreamWaitEvent(sp.stream, s->allmain_event, 0));
        TRY(launch_any(s, io, sp, m.with(PH_GRAD, &s->group_slot[gi])));
    }
    s->pending = true;
    TRY(join_groups(s, st));
    HIPCHK(hipStreamWaitEvent(st, s->cont_event, 0));
    return guard.done();
}

// fork: every group waits for what the caller's stream holds (the inputs); group g of this call runs behind group g of
// the previous call on the same internal stream.  join: the caller's stream waits for all groups -- unless the handle
// is asynchronous (dojo_set_async), where consecutive calls chain per group and dojo_join() does it once.
int step_plain_groups(DojoSim* s, const StepIO& io, hipStream_t st, size_t NG) {
    TRY(ensure_groups(s, NG));
    const Partition P(s->B, NG);
    // per-group chaining needs the same partition as the call still in flight: group g must cover the environments group g
    // covered.  Options, refinement or the group count may have changed it -- then everything in flight is joined first.
    if (s->pending && s->last_part != P) TRY(join_groups(s, st));
    s->last_part = P;
    ForkGuard guard{s, st};
    HIPCHK(hipEventRecord(s->fork_event, st));
    // Pipelined groups (dojo_set_async(h, 2), plain solves): the IFT kernel of a group's step k goes onto the group's SECOND stream, behind its
    // step kernel and next to the step kernel of step k + 1 -- both depend on step k alone.  Step k + 1 writes the other hand-off record; step
    // k + 2 re-uses record k's and waits for IFT k.  What this buys: while a group's step kernel drains (its launch lasts as long as its slowest
    // wavefront) the group has another kernel ready for the SIMDs that fall idle -- with 16 groups x 64 wavefronts = 1024 SIMDs there is no other
    // work to fill them.  The caller's inputs of un-joined calls stay untouched (the asynchronous contract): the IFT of step k reads z, u of step k.
    const bool piped = s->async == 2 && io.dz != nullptr && !std::isfinite(refine_threshold(s));
    if (piped) { TRY(ensure_pipe(s, NG)); s->sol_cur ^= 1; }
    const Mode m = step_mode(s, NG);
    for (size_t gi = 0; gi < P.groups(); ++gi) {
        const Span sp = P.span(gi, s->gstreams[gi]);
        int slot = -1;
        HIPCHK(hipStreamWaitEvent(sp.stream, s->fork_event, 0));
        if (!piped) { TRY(launch_any(s, io, sp, m.with(PH_ALL, &slot))); continue; }
        HIPCHK(hipStreamWaitEvent(sp.stream, s->grad_done[m.rec][gi], 0));      // (the IFT that read this record two calls ago)
        TRY(launch_any(s, io, sp, m.with(PH_MAIN, &slot)));
        HIPCHK(hipEventRecord(s->main_events[gi], sp.stream));
        const Span sp2{sp.env0, sp.nenv, s->gstreams2[gi % s->gstreams2.size()]};
        HIPCHK(hipStreamWaitEvent(sp2.stream, s->main_events[gi], 0));
        TRY(launch_any(s, io, sp2, m.with(PH_GRAD, &slot)));
        HIPCHK(hipEventRecord(s->grad_done[m.rec][gi], sp2.stream));
    }
    s->pending = true;
    if (!s->async) TRY(join_groups(s, st));
    return guard.done();      // (a failure: the groups already launched stay ordered before the caller's stream)
}

// RCCL, opened on first use (dojo_comm_*)
namespace rccl {
typedef struct { char internal[128]; } UniqueId;
typedef int (*get_unique_id_t)(UniqueId*);
typedef int (*comm_init_rank_t)(void**, int, UniqueId, int);
typedef int (*all_gather_t)(const void*, void*, size_t, int /*ncclDataType_t*/, void*, hipStream_t);
typedef int (*comm_destroy_t)(void*);
typedef const char* (*get_error_string_t)(int);
get_unique_id_t get_unique_id = nullptr; comm_init_rank_t comm_init_rank = nullptr; all_gather_t all_gather = nullptr;
comm_destroy_t comm_destroy = nullptr; get_error_string_t get_error_string = nullptr;
bool load() {
    static std::mutex m; std::lock_guard<std::mutex> g(m);
    if (all_gather) return true;
    void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("/opt/rocm/lib/librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) { g_err = std::string("cannot load librccl: ") + dlerror(); return false; }
    get_unique_id = (get_unique_id_t)dlsym(h, "ncclGetUniqueId"); comm_init_rank = (comm_init_rank_t)dlsym(h, "ncclCommInitRank");
    comm_destroy = (comm_destroy_t)dlsym(h, "ncclCommDestroy"); get_error_string = (get_error_string_t)dlsym(h, "ncclGetErrorString");
    all_gather_t ag = (all_gather_t)dlsym(h, "ncclAllGather");
    if (!get_unique_id || !comm_init_rank || !comm_destroy || !ag) { g_err = "librccl lacks ncclGetUniqueId / ncclCommInitRank / ncclAllGather"; return false; }
    all_gather = ag;
    return true;
}
const char* why(int rc) { return get_error_string ? get_error_string(rc) : "RCCL error"; }
}

// dojo_rollout_adjoint_dev: the reverse sweep over recorded Jacobians (dojo_adjoint.hpp), one workgroup per environment, one launch
template <class TIO>
int launch_adjoint(const DojoSim* s, int H, const void* DZ, const void* DU, const void* G, int cot_space, const void* Z, const int* status, void* gU, void* gz, hipStream_t st) {
    const dj::adjoint::Args<TIO> A{(const TIO*)DZ, (const TIO*)DU, (const TIO*)G, (const TIO*)Z, status, (TIO*)gU, (TIO*)gz, H, s->B, 12 * s->M.Nb, (int)s->M.nu, cot_space};
    hipLaunchKernelGGL((dj::adjoint::rollout_adjoint_kernel<TIO>), dim3((unsigned)s->B), dim3(dj::adjoint::THREADS), dj::adjoint::lds_bytes(A.nx), st, A);
    HIPCHK(hipGetLastError());
    return DOJO_OK;
}

// dojo_rollout_policy_dev: the controller between two steps of an environment group (dojo_policy.hpp) -- o = get_state of z, written to `obs` (null = not
// recorded), u = U_ff + E (bias + W ((o - mean) .* scale)) written to `u` (null: the observation alone).  csg: the handle's [s; gamma] of the previous step, null = the neutral 1.0.
// All pointers are batch-level; the launch covers the span's environments on the span's stream.
template <class TIO>
int launch_policy(const DojoSim* s, const DojoPolicy& p, const void* z, const void* csg, const void* uff, void* obs, void* u, const Span& sp) {
    const int Nc = p.contact_forces ? s->M.Nc : 0, nobs = 2 * s->M.nu + Nc;
    const dj::policy::Args<TIO> A{(const dj::NodeP<double>*)s->d_nodes, (const TIO*)z, (const TIO*)csg, (const TIO*)p.W, (const TIO*)p.bias, (const TIO*)p.mean, (const TIO*)p.scale,
                                  (const TIO*)uff, (TIO*)obs, (TIO*)u, (int)sp.env0, sp.nenv, s->M.Nb, s->M.nu, Nc, nobs, p.act_off, p.na, p.per_env ? 1 : 0, s->M.dt};
    hipLaunchKernelGGL((dj::policy::rollout_policy_kernel<TIO>), dim3((unsigned)((sp.nenv + dj::policy::ENVS - 1) / dj::policy::ENVS)), dim3(dj::policy::THREADS),
                       dj::policy::lds_bytes(nobs), sp.stream, A);
    HIPCHK(hipGetLastError());
    return DOJO_OK;
}
// dojo_observation_jacobian_dev: M [n][B][2nu][24] of the states (z_first; z_rest[0 .. n-2]), one launch over all (state, environment, joint) triples
int launch_observation_jacobian(const DojoSim* s, const void* z_first, const void* z_rest, long long n, double* M, hipStream_t st) {
    return by_dtype(s, [&](auto t) {
        using TIO = decltype(t);
        return launch_items(dj::padjoint::observation_jacobian_kernel<TIO>, n * s->B * s->M.Nb, dj::padjoint::JAC_THREADS, st, node_table(s), s->M.Nb, (int)s->M.nu, s->M.dt, s->B, n,
                            (const TIO*)z_first, (const TIO*)z_rest, M);
    });
}
// what the two closed-loop sweeps are given alike (padjoint::Common), from the ABI records of either entry: a is a DojoPolicyAdjoint or a DojoMlpAdjoint, p its policy
template <class TIO, class Rec, class Pol>
dj::padjoint::Common<TIO> closed_loop_common(const DojoSim* s, const Pol& p, int H, const Rec& a, const double* M) {
    dj::padjoint::Common<TIO> c{};
    c.DZ = (const TIO*)a.DZ; c.DU = (const TIO*)a.DU; c.OBS = (const TIO*)a.OBS; c.M = M; c.G = (const TIO*)a.G; c.Z = (const TIO*)a.Z;
    c.G_u = (const TIO*)a.G_u; c.G_obs = (const TIO*)a.G_obs; c.status = a.status; c.mean = (const TIO*)p.mean; c.scale = (const TIO*)p.scale;
    c.touch = dj::padjoint::Touch{s->d_touch_ptr, s->d_touch_ent};
    c.gU = (TIO*)a.gU; c.gz = (TIO*)a.gz;
    c.H = H; c.B = s->B; c.nx = 12 * s->M.Nb; c.nu = (int)s->M.nu; c.nobs = 2 * c.nu; c.act_off = p.act_off; c.per_env = p.per_env ? 1 : 0; c.cot_space = a.cot_space;
    return c;
}
// shared policy: the sum over the batch of the per-environment accumulators acc [B][nacc]; the entries [0, nW) go to gW, the rest to gbias (each may be null)
template <class TIO>
int launch_policy_reduce(const DojoSim* s, const double* acc, int nacc, int nW, void* gW, void* gbias, hipStream_t st) {
    const int per = dj::padjoint::THREADS / dj::adjoint::ROW;
    hipLaunchKernelGGL((dj::padjoint::policy_reduce_kernel<TIO>), dim3((unsigned)((nacc + per - 1) / per)), dim3(dj::padjoint::THREADS), 0, st, acc, s->B, nacc, nW, (TIO*)gW, (TIO*)gbias);
    HIPCHK(hipGetLastError());
    return DOJO_OK;
}
// dojo_rollout_policy_adjoint_dev: the closed-loop reverse sweep (one workgroup per environment, one launch) and, for a shared policy, the reduction over the batch
template <class TIO>
int launch_policy_adjoint(const DojoSim* s, const DojoPolicy& p, int H, const DojoPolicyAdjoint& a, const double* M, double* acc, hipStream_t st) {
    dj::padjoint::Args<TIO> A{};
    A.c = closed_loop_common<TIO>(s, p, H, a, M);
    A.W = (const TIO*)p.W; A.gW = acc ? nullptr : (TIO*)a.gW; A.gbias = acc ? nullptr : (TIO*)a.gbias; A.acc_out = acc; A.na = p.na;
    hipLaunchKernelGGL((dj::padjoint::rollout_policy_adjoint_kernel<TIO>), dim3((unsigned)s->B), dim3(dj::padjoint::THREADS), dj::padjoint::lds_bytes(A.c.nx, A.c.nu, A.c.nobs, A.na), st, A);
    HIPCHK(hipGetLastError());
    return acc ? launch_policy_reduce<TIO>(s, acc, A.na * (A.c.nobs + 1), A.na * A.c.nobs, a.gW, a.gbias, st) : DOJO_OK;
}
// a workspace of the handle whose size depends on the call: kept while it is large enough, replaced (hipFree waits for the device) when it is not
int ensure_at_least(DojoSim* s, void** p, size_t* have, size_t bytes) {
    if (*p && *have >= bytes) return DOJO_OK;
    if (s->measure) { *s->measure += granules(bytes); return DOJO_OK; }
    if (*p) { s->owned.erase(std::remove(s->owned.begin(), s->owned.end(), *p), s->owned.end()); HIPCHK(hipFree(*p)); *p = nullptr; *have = 0; }
    HIPCHK(hipMalloc(p, bytes ? bytes : 8));
    s->owned.push_back(*p); *have = bytes;
    return DOJO_OK;
}
// ... those of the sweeps: the observation Jacobians of a closed-loop sweep whose caller passes none, and the per-environment accumulators in front of a reduction over the batch
size_t pM_size(const DojoSim* s, size_t H) { return (H + 1) * s->B * 2 * s->M.nu * 24 * sizeof(double); }
size_t macc_size(const DojoSim* s, size_t P) { return (size_t)s->B * P * sizeof(double); }
int ensure_pM(DojoSim* s, size_t H) { return ensure_at_least(s, &s->d_pM, &s->pM_bytes, pM_size(s, H)); }
int ensure_pacc(DojoSim* s, size_t na) { return ensure_at_least(s, (void**)&s->d_pacc, &s->pacc_bytes, (size_t)s->B * na * (2 * s->M.nu + 1) * sizeof(double)); }
int ensure_macc(DojoSim* s, size_t P) { return ensure_at_least(s, (void**)&s->d_macc, &s->macc_bytes, macc_size(s, P)); }
int ensure_dacc(DojoSim* s) { return ensure_at_least(s, (void**)&s->d_dacc, &s->dacc_bytes, (size_t)s->B * 5 * s->M.Nc * sizeof(double)); }

// The temporary device buffers of a host-pointer rollout entry.  Each is declared once -- its size, the host array uploaded into it, the host array it is downloaded
// into (either may be none) -- before anything is allocated, so that bytes() is the total of exactly what allocate() takes; all are freed on every return path.
struct Staging {
    struct Buf { size_t bytes; const void* src; void* dst; void* p; };
    std::deque<Buf> bufs;               // (a deque: the references handed out stay valid)
    Staging() = default; Staging(const Staging&) = delete; Staging& operator=(const Staging&) = delete;
    ~Staging() { for (Buf& b : bufs) if (b.p) (void)hipFree(b.p); }
    const Buf& input(size_t bytes, const void* src) { return add(bytes, src, nullptr, src != nullptr); }      // uploaded; a NULL array: no buffer
    const Buf& output(size_t bytes, void* dst) { return add(bytes, nullptr, dst, dst != nullptr); }           // downloaded; a NULL array: no buffer
    const Buf& kept(size_t bytes, void* dst = nullptr, bool wanted = true) { return add(bytes, nullptr, dst, wanted); }      // the device side needs it either way; downloaded into a non-NULL array
    size_t bytes() const { size_t n = 0; for (const Buf& b : bufs) n += granules(b.bytes); return n; }
    int allocate() {
        for (Buf& b : bufs) {
            HIPCHK(hipMalloc(&b.p, b.bytes ? b.bytes : 8));
            if (b.src) HIPCHK(hipMemcpy(b.p, b.src, b.bytes, hipMemcpyHostToDevice));
        }
        return DOJO_OK;
    }
    // behind the device work of the call: the downloads ...
    int finish() {
        HIPCHK(hipDeviceSynchronize());
        for (const Buf& b : bufs) if (b.dst) HIPCHK(hipMemcpy(b.dst, b.p, b.bytes, hipMemcpyDeviceToHost));
        return DOJO_OK;
    }
    // ... and, of a rollout, the last state Z[H-1] into the handle's d_zn (dojo_get_state) as a rollout without Z leaves it there
    int finish(DojoSim* s, const Buf& Z, int H) {
        TRY(finish());
        const size_t zb = (size_t)s->B * 13 * s->M.Nb * s->w;
        if (Z.p) HIPCHK(hipMemcpy(s->d_zn, (char*)Z.p + (size_t)(H - 1) * zb, zb, hipMemcpyDeviceToDevice));
        return DOJO_OK;
    }
private:
    const Buf& add(size_t bytes, const void* src, void* dst, bool wanted) {
        static const Buf none{0, nullptr, nullptr, nullptr};
        if (!wanted) return none;
        bufs.push_back(Buf{bytes, src, dst, nullptr});
        return bufs.back();
    }
};

// The host-pointer step entries keep their arrays in buffers of the handle instead: those are state (dojo_gradients and dojo_contact_gradients read d_z, d_u and
// d_dz later) and a step must not pay for allocations.  In front of the step: the state (n scalars per environment) into d_state and, for an entry with controls
// (d_u given), the controls into the handle's d_u -- *d_u: where they are, null where the call has none.
int upload_step(DojoSim* s, void* d_state, const void* state, size_t n, const void* u = nullptr, const void** d_u = nullptr) {
    const size_t B = s->B, w = s->w, nu = s->M.nu;
    ENSURE(s->d_status, B * sizeof(int)); ENSURE(s->d_iters, B * sizeof(int));
    HIPCHK(hipMemcpy(d_state, state, B * n * w, hipMemcpyHostToDevice));
    if (!d_u) return DOJO_OK;
    ENSURE(s->d_u, B * (nu + 1) * w);
    *d_u = (u && nu) ? s->d_u : nullptr;
    if (*d_u) HIPCHK(hipMemcpy(s->d_u, u, B * nu * w, hipMemcpyHostToDevice));
    return DOJO_OK;
}
// Behind it: the next state (n scalars per environment, from d_next) and the handle's d_status / d_iters into the arrays that are wanted
int download_step(DojoSim* s, void* next, const void* d_next, size_t n, int32_t* status, int32_t* iters) {
    const size_t B = s->B;
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(next, d_next, B * n * s->w, hipMemcpyDeviceToHost));
    if (status) HIPCHK(hipMemcpy(status, s->d_status, B * sizeof(int), hipMemcpyDeviceToHost));
    if (iters) HIPCHK(hipMemcpy(iters, s->d_iters, B * sizeof(int), hipMemcpyDeviceToHost));
    return DOJO_OK;
}
// The device keeps Jacobians column-major per environment (Julia-native), the host ABI is row-major: dst [B][rows][cols] on the host <- src [B][cols][rows] on the device
int download_transposed(const DojoSim* s, void* dst, const void* src, size_t rows, size_t cols) {
    const size_t B = s->B, w = s->w;
    std::vector<char> tmp(B * rows * cols * w);
    HIPCHK(hipMemcpy(tmp.data(), src, tmp.size(), hipMemcpyDeviceToHost));
    for (size_t b = 0; b < B; ++b)
        for (size_t c = 0; c < cols; ++c)
            for (size_t r = 0; r < rows; ++r)
                std::memcpy((char*)dst + ((b * rows + r) * cols + c) * w, tmp.data() + ((b * cols + c) * rows + r) * w, w);
    return DOJO_OK;
}

// dojo_rollout_data_adjoint_dev: the contact-data sweep (dojo_data_adjoint.hpp; one workgroup per environment, one launch) and, for the gradient shared by the
// batch, the reduction over the environments (one workgroup per entry)
template <class TIO>
int launch_data_adjoint(const DojoSim* s, int H, const void* DZ, const void* DC, const void* G, int cot_space, const void* Z, const int* status, void* gtheta_env, double* acc,
                        void* gtheta, void* gz, hipStream_t st) {
    const int nx = 12 * s->M.Nb, nth = 5 * s->M.Nc;
    const dj::dadjoint::Args<TIO> A{(const TIO*)DZ, (const TIO*)DC, (const TIO*)G, (const TIO*)Z, status, (TIO*)gtheta_env, acc, (TIO*)gz, H, s->B, nx, nth, cot_space};
    hipLaunchKernelGGL((dj::dadjoint::rollout_data_adjoint_kernel<TIO>), dim3((unsigned)s->B), dim3(dj::dadjoint::THREADS), dj::dadjoint::lds_bytes(nx, nth), st, A);
    HIPCHK(hipGetLastError());
    if (acc) {
        hipLaunchKernelGGL((dj::dadjoint::data_reduce_kernel<TIO>), dim3((unsigned)nth), dim3(dj::dadjoint::THREADS), 0, st, (const double*)acc, s->B, nth, (TIO*)gtheta);
        HIPCHK(hipGetLastError());
    }
    return DOJO_OK;
}

// dojo_rollout_tangent_dev: the forward sweep over recorded Jacobians (dojo_tangent.hpp), one workgroup per environment and chunk of NT tangents, one launch
template <class TIO>
int launch_tangent(const DojoSim* s, int H, int T, const void* DZ, const void* DU, const void* DC, const void* dz0, const void* dU, const void* dth, int tan_space, const void* Z,
                   const int* status, void* dZ, hipStream_t st) {
    const int nx = 12 * s->M.Nb, nu = (int)s->M.nu, nth = 5 * s->M.Nc, nchunk = (T + dj::tangent::NT - 1) / dj::tangent::NT;
    const dj::tangent::Args<TIO> A{(const TIO*)DZ, (const TIO*)DU, (const TIO*)DC, (const TIO*)dz0, (const TIO*)dU, (const TIO*)dth, (const TIO*)Z, status, (TIO*)dZ, H, s->B, T, nx, nu, nth, tan_space};
    hipLaunchKernelGGL((dj::tangent::rollout_tangent_kernel<TIO>), dim3((unsigned)((size_t)s->B * nchunk)), dim3(dj::tangent::THREADS), dj::tangent::lds_bytes(nx, nu, nth, sizeof(TIO)), st, A);
    HIPCHK(hipGetLastError());
    return DOJO_OK;
}

// what dojo_riccati_box_dev takes on top of the DojoRiccati record (include/dojo_hip_limits.h); null in its place: the unconstrained pass
struct RiccatiBox { const DojoControlLimits* lim; const void* U; int64_t* active; int32_t* qp_iters; };
// ... and what dojo_riccati_al_dev takes on top of that (include/dojo_hip_constraints.h); with it lim and U of the box may be null
using RiccatiCon = DojoStageConstraints;

// dojo_riccati_dev, dojo_riccati_box_dev, dojo_riccati_al_dev: the Riccati backward pass (dojo_riccati.hpp), one workgroup per environment, one launch; NQ = register accumulators per lane
template <class TIO, int NQ>
int launch_riccati(const DojoSim* s, int H, const DojoRiccati& r, const RiccatiBox* box, const RiccatiCon* con, hipStream_t st) {
    const int nu = (int)s->M.nu, n = 2 * nu;
    const dj::riccati::Args<TIO> A{(const TIO*)r.A, (const TIO*)r.Bm, r.status, (const TIO*)r.lx, (const TIO*)r.lu, (const TIO*)r.lxx, (const TIO*)r.luu, (const TIO*)r.lux, (const TIO*)r.mu,
                                   (TIO*)r.K, (TIO*)r.kff, r.fail, (TIO*)r.dV, (TIO*)r.Vx, (TIO*)r.Vxx, H, s->B, n, nu, r.na, r.act_off};
    if (box) {
        dj::riccati::AlArgs<TIO> al{}; dj::riccati::BoxArgs<TIO>& bx = al; static_cast<dj::riccati::Args<TIO>&>(bx) = A;
        bx.lo = (const TIO*)(box->lim ? box->lim->lo : nullptr); bx.hi = (const TIO*)(box->lim ? box->lim->hi : nullptr); bx.U = (const TIO*)box->U;
        bx.active = (long long*)box->active; bx.iters = box->qp_iters;
        if (con && (con->nc > 0 || !box->U)) {       // (no rows: the control-limited kernel is the constrained one's bits and has fewer registers; it needs U, though)
            al.Cx = (const TIO*)con->Cx; al.Cu = (const TIO*)con->Cu; al.w = (const TIO*)con->w; al.y = (const TIO*)con->y; al.nc = con->nc; al.shared = con->shared;
            hipLaunchKernelGGL((dj::riccati::riccati_kernel<TIO, NQ, dj::riccati::AlArgs<TIO>>), dim3((unsigned)s->B), dim3(dj::riccati::THREADS), dj::riccati::al_lds_bytes(n, r.na), st, al);
        } else
            hipLaunchKernelGGL((dj::riccati::riccati_kernel<TIO, NQ, dj::riccati::BoxArgs<TIO>>), dim3((unsigned)s->B), dim3(dj::riccati::THREADS), dj::riccati::box_lds_bytes(n, r.na), st, bx);
    } else
        hipLaunchKernelGGL((dj::riccati::riccati_kernel<TIO, NQ>), dim3((unsigned)s->B), dim3(dj::riccati::THREADS), dj::riccati::lds_bytes(n, r.na), st, A);
    HIPCHK(hipGetLastError());
    return DOJO_OK;
}
template <class TIO>
int launch_riccati_any(const DojoSim* s, int H, const DojoRiccati& r, const RiccatiBox* box, const RiccatiCon* con, hipStream_t st) {
    switch (dj::riccati::accumulators(2 * (int)s->M.nu, r.na)) {
        case 3: return launch_riccati<TIO, 3>(s, H, r, box, con, st);
        case 6: return launch_riccati<TIO, 6>(s, H, r, box, con, st);
        case 12: return launch_riccati<TIO, 12>(s, H, r, box, con, st);
        default: return launch_riccati<TIO, 24>(s, H, r, box, con, st);
    }
}

int launch_policy_any(const DojoSim* s, const DojoPolicy& p, const void* z, const void* csg, const void* uff, void* obs, void* u, const Span& sp) {
    return by_dtype(s, [&](auto t) { return launch_policy<decltype(t)>(s, p, z, csg, uff, obs, u, sp); });
}

// dojo_rollout_mlp_dev: the same controller with a tanh network in place of the mat-vec (dojo_mlp.hpp); act: [B][nh] of this step or null
template <class TIO>
int launch_mlp(const DojoSim* s, const DojoMlpPolicy& p, const dj::mlp::Shape& sh, const void* z, const void* csg, const void* uff, void* obs, void* u, double* act, const Span& sp) {
    const int Nc = p.contact_forces ? s->M.Nc : 0, nobs = 2 * s->M.nu + Nc;
    const dj::mlp::Args<TIO> A{(const dj::NodeP<double>*)s->d_nodes, (const TIO*)z, (const TIO*)csg, (const TIO*)p.theta, (const TIO*)p.mean, (const TIO*)p.scale,
                               (const TIO*)uff, (TIO*)obs, (TIO*)u, act, (int)sp.env0, sp.nenv, s->M.Nb, s->M.nu, Nc, nobs, p.act_off, p.per_env ? 1 : 0, (int)sh.P, s->M.dt, sh};
    hipLaunchKernelGGL((dj::mlp::rollout_mlp_kernel<TIO>), dim3((unsigned)((sp.nenv + dj::policy::ENVS - 1) / dj::policy::ENVS)), dim3(dj::policy::THREADS),
                       dj::mlp::lds_bytes(nobs, sh.nh), sp.stream, A);
    HIPCHK(hipGetLastError());
    return DOJO_OK;
}

// dojo_rollout_minimal_dev: the tracking controller of step k on the environments and the stream of `sp`.  z: the state the previous step left, or -- k = 0 -- the
// initial MINIMAL state; x: X[k]; zproj: where the re-projected state goes, which step k reads.  X[k] by max2min_kernel (k = 0: a copy), the control law
// (dojo_tracking.hpp), the re-projection by min2max_kernel: the two maps are the kernels of dojo_step_minimal_dev, which index environments from 0 and are given
// the span's slice of every array.  The observation of the final state (u = null) is the first of the three alone.
template <class TIO>
int launch_tracking(const DojoSim* s, const DojoTracking& t, const DojoControlLimits* lim, int fan_P, int k, const void* z, const void* uff, void* x, void* u, void* zproj, const Span& sp) {
    // fan_P > 0 (dojo_rollout_minimal_fan_dev): the reference members hold P = fan_P rows per step, not B, and x0 is [P][n]
    const size_t B = s->B, Nb = s->M.Nb, nu = s->M.nu, n = 2 * nu, kB = (size_t)k * (fan_P ? (size_t)fan_P : B), e0 = sp.env0;
    TIO* const xs = (TIO*)x + e0 * n;
    if (k == 0 && fan_P) {
        // X[0][tr P + p] = x0[p]: the span's environments piece by piece, a piece ending where a trial ends (a span may begin and end inside a trial)
        for (size_t e = e0, end = e0 + (size_t)sp.nenv; e < end;) {
            const size_t p = e % (size_t)fan_P, cnt = std::min(end - e, (size_t)fan_P - p);
            HIPCHK(hipMemcpyAsync((TIO*)x + e * n, (const TIO*)z + p * n, cnt * n * sizeof(TIO), hipMemcpyDeviceToDevice, sp.stream));
            e += cnt;
        }
    }
    else if (k == 0) HIPCHK(hipMemcpyAsync(xs, (const TIO*)z + e0 * n, (size_t)sp.nenv * n * sizeof(TIO), hipMemcpyDeviceToDevice, sp.stream));
    else TRY(launch_items(dj::ckern::max2min_kernel<TIO>, (long long)sp.nenv * Nb, 256, sp.stream, node_table(s), (int)Nb, (int)nu, s->M.dt, sp.nenv, (const TIO*)z + e0 * 13 * Nb, xs, (int)n));
    if (!u) return DOJO_OK;
    auto row = [&](const void* p, size_t per) { return p ? (const TIO*)p + kB * per : nullptr; };      // step k of an input that is given
    // (the fan's Ubar has P rows per step as well: rollout_core, which strides by B, is not given it -- uff is null then)
    const dj::tracking::Args<TIO> A{(const TIO*)x, fan_P ? row(t.Ubar, nu) : (const TIO*)uff, row(t.Xbar, n), row(t.K, (size_t)t.na * n), row(t.kff, (size_t)t.na), (const TIO*)t.alpha, (TIO*)u,
                                    (int)sp.env0, sp.nenv, (int)nu, t.act_off, t.na};
    const dim3 grid((unsigned)((sp.nenv + dj::policy::ENVS - 1) / dj::policy::ENVS));
    if (fan_P) {     // (dojo_rollout_minimal_fan_dev; lim null: no limits)
        dj::tracking::FanArgs<TIO> fa; static_cast<dj::tracking::Args<TIO>&>(fa) = A;
        fa.lo = lim ? (const TIO*)lim->lo : nullptr; fa.hi = lim ? (const TIO*)lim->hi : nullptr; fa.P = fan_P;
        hipLaunchKernelGGL((dj::tracking::rollout_tracking_kernel<TIO, dj::tracking::FanArgs<TIO>>), grid, dim3(dj::policy::THREADS), 0, sp.stream, fa);
    }
    else if (lim) {  // (dojo_rollout_minimal_box_dev)
        dj::tracking::BoxArgs<TIO> bx; static_cast<dj::tracking::Args<TIO>&>(bx) = A; bx.lo = (const TIO*)lim->lo; bx.hi = (const TIO*)lim->hi;
        hipLaunchKernelGGL((dj::tracking::rollout_tracking_kernel<TIO, dj::tracking::BoxArgs<TIO>>), grid, dim3(dj::policy::THREADS), 0, sp.stream, bx);
    }
    else hipLaunchKernelGGL((dj::tracking::rollout_tracking_kernel<TIO>), grid, dim3(dj::policy::THREADS), 0, sp.stream, A);
    HIPCHK(hipGetLastError());
    return launch_items(dj::ckern::min2max_kernel<TIO>, sp.nenv, 64, sp.stream, node_table(s), (const int*)s->d_order, (int)Nb, (int)nu, s->M.dt, sp.nenv, (const TIO*)xs, (TIO*)zproj + e0 * 13 * Nb);
}

// The controller of a closed-loop rollout, as rollout_core sees it: the affine policy, the network or the tracking controller of a rollout in minimal coordinates
// (exactly one is set), and what the network records
struct Controller {
    const DojoPolicy* affine = nullptr;
    const DojoMlpPolicy* mlp = nullptr;
    const DojoTracking* tracking = nullptr;
    const DojoControlLimits* limits = nullptr;     // of the tracking controller (dojo_rollout_minimal_box_dev) or null
    int fan_P = 0;                                 // of the tracking controller: > 0 = the fan of dojo_rollout_minimal_fan_dev over P problems (include/dojo_hip_linesearch.h)
    dj::mlp::Shape shape{};
    double* ACT = nullptr;              // [H][B][nh] or null
    bool contact_forces() const { return tracking ? false : affine ? affine->contact_forces != 0 : mlp->contact_forces != 0; }
    bool contact_init() const { return tracking ? false : affine ? affine->contact_init != 0 : mlp->contact_init != 0; }
};
// the controls of step k (u != null) or the observation of the final state (u = null, k = H).  zproj: the tracking controller's re-projected state (the others make none)
int launch_controller(const DojoSim* s, const Controller& c, int k, const void* z, const void* csg, const void* uff, void* obs, void* u, const Span& sp, void* zproj = nullptr) {
    if (c.tracking) return by_dtype(s, [&](auto t) { return launch_tracking<decltype(t)>(s, *c.tracking, c.limits, c.fan_P, k, z, uff, obs, u, zproj, sp); });
    if (c.affine) return launch_policy_any(s, *c.affine, z, csg, uff, obs, u, sp);
    double* const act = (c.ACT && u) ? c.ACT + (size_t)k * s->B * c.shape.nh : nullptr;
    return by_dtype(s, [&](auto t) { return launch_mlp<decltype(t)>(s, *c.mlp, c.shape, z, csg, uff, obs, u, act, sp); });
}

// dojo_rollout_mlp_adjoint_dev: the sweep (one workgroup per environment, one launch) and, for a shared policy, the reduction over the batch
template <class TIO>
int launch_mlp_adjoint(const DojoSim* s, const DojoMlpPolicy& p, const dj::mlp::Shape& sh, int H, const DojoMlpAdjoint& a, const double* M, double* ws, hipStream_t st) {
    dj::mlp::AdjointArgs<TIO> A{};
    A.c = closed_loop_common<TIO>(s, p, H, a, M);
    A.ACT = a.ACT; A.theta = (const TIO*)p.theta; A.ws = ws; A.gtheta = (TIO*)a.gtheta; A.shared = p.per_env ? 0 : 1; A.P = (int)sh.P; A.s = sh;
    hipLaunchKernelGGL((dj::mlp::rollout_mlp_adjoint_kernel<TIO>), dim3((unsigned)s->B), dim3(dj::padjoint::THREADS), dj::mlp::adjoint_lds_bytes(A.c.nx, A.c.nu, A.c.nobs, sh.wmax, sh.nh), st, A);
    HIPCHK(hipGetLastError());
    // at n_layers = 1 theta is [W | bias], the order of the affine sweep's accumulators: every entry goes to the one output
    return (!p.per_env && a.gtheta) ? launch_policy_reduce<TIO>(s, ws, (int)sh.P, (int)sh.P, a.gtheta, nullptr, st) : DOJO_OK;
}

// dojo_linesearch_select_dev: one workgroup per problem (dojo_linesearch.hpp)
template <class TIO>
int launch_select(const DojoSim* s, int H, int T, const DojoQuadraticCost* cost, const DojoLineSearch& l, hipStream_t st) {
    dj::linesearch::Args<TIO> A{};
    A.X = (const TIO*)l.X; A.U = (const TIO*)l.U; A.status = l.status; A.alpha = (const TIO*)l.alpha; A.dV = (const TIO*)l.dV; A.ok = l.ok;
    A.Xcur = (const TIO*)l.Xcur; A.Ucur = (const TIO*)l.Ucur; A.J0 = l.J0; A.J_trial = l.J_trial; A.J_cur = l.J_cur; A.J_acc = l.J_acc;
    A.choice = l.choice; A.alpha_acc = (TIO*)l.alpha_acc; A.X_new = (TIO*)l.X_new; A.U_new = (TIO*)l.U_new;
    if (cost) { A.Q = (const TIO*)cost->Q; A.R = (const TIO*)cost->R; A.Qf = (const TIO*)cost->Qf; A.goal = (const TIO*)cost->goal; A.goal_per_problem = cost->goal_per_problem ? 1 : 0; }
    A.c1 = l.c1; A.H = H; A.T = T; A.P = (int)(s->B / (size_t)T); A.nu = (int)s->M.nu; A.act_off = l.act_off; A.na = l.na;
    hipLaunchKernelGGL((dj::linesearch::linesearch_select_kernel<TIO>), dim3((unsigned)A.P), dim3(dj::linesearch::THREADS), 0, st, A);
    HIPCHK(hipGetLastError());
    return DOJO_OK;
}

} // namespace

extern "C" {

const char* dojo_last_error(void) { return g_err.c_str(); }
// text of the last failure of a call on THIS handle ("" if none); the pointer stays valid until the next failing call on it
const char* dojo_handle_error(DojoHandle s) { if (!s) return ""; std::lock_guard<std::mutex> g(s->err_m); return s->err.c_str(); }

int dojo_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

void dojo_destroy(DojoHandle s);

int dojo_create(const DojoTopology* topo, int32_t batch, int32_t dtype, int32_t device, DojoHandle* out) {
    if (!topo || !out || batch < 1 || (dtype != DOJO_DTYPE_F64 && dtype != DOJO_DTYPE_F32)) { g_err = "dojo_create: bad argument"; return DOJO_ERR_INVALID; }
    int ndev = dojo_device_count();
    if (ndev <= 0) { g_err = "no HIP device visible: libdojo_hip has no CPU fallback"; return DOJO_ERR_NO_DEVICE; }
    if (device < 0 || device >= ndev) { g_err = "dojo_create: device index out of range"; return DOJO_ERR_INVALID; }
    DojoSim* s = new DojoSim();
    int rc = dj::build_host_model(*topo, s->M);
    if (rc != DOJO_OK) { g_err = s->M.error; delete s; return rc; }
    if (s->M.has_ss && s->M.contact_model != 2 && (mapping_waves(s->M) != 1 || s->M.maxc > 1 || s->M.has_tsd || s->M.has_mlim || s->M.has_cut)) {
        // the tree-edge builds (k_*_1_1_ss) do not serve this mechanism: the contact travels as a cut element of the general lane-mapping builds
        rc = dj::promote_tree_edge_contacts(s->M);
        if (rc != DOJO_OK) { g_err = s->M.error; delete s; return rc; }
    }
    if (s->M.has_ss && (mapping_waves(s->M) != 1 || s->M.maxc > 1 || s->M.has_tsd)) {
        g_err = "a LinearContact body-body contact needs the single-wavefront quad mapping (<= 16 bodies), at most one contact per body and no translational springs / dampers / limits"; delete s; return DOJO_ERR_UNSUPPORTED;
    }
    if ((s->M.has_mlim || s->M.has_cut) && (s->M.contact_model == 2 || s->M.has_ss)) {   // (has_ss: a body-body contact along a tree edge -- the quad builds; next to cut elements: not built)
        g_err = "joint limits on several coordinates / both halves, or a kinematic loop, together with LinearContact or a body-body contact are not supported (no kernel build carries both)"; delete s; return DOJO_ERR_UNSUPPORTED;
    }
    if (s->M.contact_model == 2 && s->M.has_tsd) {
        g_err = "LinearContact together with translational springs / dampers / limits is not supported (no kernel build carries both)"; delete s; return DOJO_ERR_UNSUPPORTED;
    }
    s->B = batch; s->dtype = dtype; s->device = device; s->w = dtype == DOJO_DTYPE_F32 ? 4 : 8;
    s->opts = dj::default_options();
    if (hipSetDevice(device) != hipSuccess) { g_err = "dojo_create: hipSetDevice failed"; delete s; return DOJO_ERR_DEVICE; }
    if (hipDeviceGetAttribute(&s->sm_count, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) s->sm_count = 0;      // (several_rounds: 256 then)
    rc = upload_tables<double>(s);
    if (rc != DOJO_OK) { dojo_destroy(s); return rc; }          // frees whatever part of the tables was uploaded
    *out = s;
    return DOJO_OK;
}

void dojo_destroy(DojoHandle s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    for (void* p : s->owned) (void)hipFree(p);
    if (s->cstream) (void)hipStreamDestroy(s->cstream);
    if (s->cont_event) (void)hipEventDestroy(s->cont_event);
    if (s->allmain_event) (void)hipEventDestroy(s->allmain_event);
    for (auto e_ : s->main_events) (void)hipEventDestroy(e_);
    for (auto g_ : s->gstreams) (void)hipStreamDestroy(g_);
    for (auto g_ : s->gstreams2) (void)hipStreamDestroy(g_);
    for (auto e_ : s->gevents2) (void)hipEventDestroy(e_);
    for (int p_ = 0; p_ < 2; ++p_) for (auto e_ : s->grad_done[p_]) (void)hipEventDestroy(e_);
    for (auto gev_ : s->gevents) (void)hipEventDestroy(gev_);
    if (s->fork_event) (void)hipEventDestroy(s->fork_event);
    if (s->comm && rccl::comm_destroy) (void)rccl::comm_destroy(s->comm);
    for (auto& e : s->ring) { if (e.a) (void)hipEventDestroy(e.a); if (e.m) (void)hipEventDestroy(e.m); if (e.b) (void)hipEventDestroy(e.b); }
    delete s;
}

int dojo_get_dims(DojoHandle s, DojoDims* d) {
    Enter enter_(s);
    if (!s || !d) { g_err = "dojo_get_dims: bad argument"; return DOJO_ERR_INVALID; }
    d->n_bodies = s->M.Nb; d->n_joints = (int)s->M.nodes.size(); d->n_contacts = s->M.Nc;
    d->nz = 13 * s->M.Nb; d->nx = 12 * s->M.Nb; d->nu = s->M.nu; d->n_joint_impulses = s->M.n_joint_imp;
    d->n_solution = s->M.n_joint_imp + 6 * s->M.Nb + csg_per(s) * s->M.Nc; d->lanes_per_env = s->M.S;
    return DOJO_OK;
}

int dojo_set_options(DojoHandle s, const DojoSolverOptions* o) {
    Enter enter_(s);
    if (!s || !o || o->max_iter < 1 || o->max_ls < 1) { g_err = "dojo_set_options: bad argument"; return DOJO_ERR_INVALID; }
    s->opts = *o; return DOJO_OK;
}

// set_external_force!(body; force, torque, vertex) (src/bodies/set.jl:110-115) for every body of every environment: state.Fext
// (world frame) and state.τext (body frame) as they enter the body residual (integrators/constraint.jl:15-18)
int dojo_set_external_force_dev(DojoHandle s, const void* fext) {
    Enter enter_(s);
    if (!s) { g_err = "dojo_set_external_force_dev: bad argument"; return DOJO_ERR_INVALID; }
    s->fext = fext;
    return DOJO_OK;
}
int dojo_set_external_force(DojoHandle s, const void* fext) {
    Enter enter_(s);
    if (!s) { g_err = "dojo_set_external_force: bad argument"; return DOJO_ERR_INVALID; }
    if (!fext) { s->fext = nullptr; return DOJO_OK; }
    HIPCHK(hipSetDevice(s->device));
    const size_t bytes = (size_t)s->B * 6 * s->M.Nb * s->w;
    ENSURE(s->d_fext, bytes);
    HIPCHK(hipDeviceSynchronize());                          // steps still in flight read the previous forces
    HIPCHK(hipMemcpy(s->d_fext, fext, bytes, hipMemcpyHostToDevice));
    s->fext = s->d_fext;
    return DOJO_OK;
}

// Accuracy of the linear solves (no counterpart in the reference, whose LDU has no such knob): environments whose cone
// variables reach max γ/s > stiffness get their Newton and IFT solves refined against the uncondensed KKT system.
// INFINITY switches the refinement off, 0 refines every solve.
int dojo_set_refinement(DojoHandle s, double stiffness) {
    Enter enter_(s);
    if (!s || stiffness != stiffness) { g_err = "dojo_set_refinement: bad argument"; return DOJO_ERR_INVALID; }   // negative: back to the tolerance-based default
    s->refine_w = stiffness; return DOJO_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Multi-GPU: one process per GPU, the batch sharded in contiguous slices, no exchange inside the solver; the
// one collective is an all-gather of per-rank outputs (final states of a rollout chunk, status, gradients when wanted) over
// RCCL / xGMI.  RCCL is opened lazily (dlopen), so a single-GPU user never loads it.  The 128-byte unique id travels over
// whatever the host already has between its processes (Julia Distributed / MPI; torch.distributed in bench.py).
// ---------------------------------------------------------------------------------------------------------------
// rank 0 creates the id (128 bytes) and the host hands it to every rank
int dojo_comm_unique_id(void* id128) {
    if (!id128) { g_err = "dojo_comm_unique_id: bad argument"; return DOJO_ERR_INVALID; }
    if (!rccl::load()) return DOJO_ERR_DEVICE;
    rccl::UniqueId id;
    int rc = rccl::get_unique_id(&id);
    if (rc != 0) { g_err = std::string("ncclGetUniqueId: ") + rccl::why(rc); return DOJO_ERR_DEVICE; }
    std::memcpy(id128, &id, 128);
    return DOJO_OK;
}
// joins the handle's device into a communicator of `world` ranks (one handle, one GPU, one process each)
int dojo_comm_init(DojoHandle s, int32_t rank, int32_t world, const void* id128) {
    Enter enter_(s);
    if (!s || !id128 || world < 1 || rank < 0 || rank >= world) { g_err = "dojo_comm_init: bad argument"; return DOJO_ERR_INVALID; }
    if (!rccl::load()) return DOJO_ERR_DEVICE;
    HIPCHK(hipSetDevice(s->device));
    if (s->comm) { HIPCHK(hipDeviceSynchronize()); (void)rccl::comm_destroy(s->comm); s->comm = nullptr; }     // (collectives of the old communicator may still be in flight)
    rccl::UniqueId id; std::memcpy(&id, id128, 128);
    int rc = rccl::comm_init_rank(&s->comm, world, id, rank);
    if (rc != 0) { s->comm = nullptr; g_err = std::string("ncclCommInitRank: ") + rccl::why(rc); return DOJO_ERR_DEVICE; }
    s->comm_rank = rank; s->comm_world = world;
    return DOJO_OK;
}
// recv[world][count] <- every rank's send[count] (scalars of the handle's dtype; int32 with as_int32), in rank order = the
// order of the contiguous batch shards.  Runs on `stream` behind everything the handle has in flight.
int dojo_allgather_dev(DojoHandle s, const void* send, void* recv, int64_t count, int32_t as_int32, void* stream) {
    Enter enter_(s);
    if (!s || !send || !recv || count < 0) { g_err = "dojo_allgather_dev: bad argument"; return DOJO_ERR_INVALID; }
    if (!s->comm) { g_err = "dojo_allgather_dev: no communicator (dojo_comm_init)"; return DOJO_ERR_INVALID; }
    HIPCHK(hipSetDevice(s->device));
    TRY(join_groups(s, (hipStream_t)stream));
    const int dt = as_int32 ? 2 /*ncclInt32*/ : (s->dtype == DOJO_DTYPE_F32 ? 7 /*ncclFloat32*/ : 8 /*ncclFloat64*/);
    int rc = rccl::all_gather(send, recv, (size_t)count, dt, s->comm, (hipStream_t)stream);
    if (rc != 0) { g_err = std::string("ncclAllGather: ") + rccl::why(rc); return DOJO_ERR_DEVICE; }
    return DOJO_OK;
}
int dojo_comm_info(DojoHandle s, int32_t* rank, int32_t* world) {
    Enter enter_(s);
    if (!s) { g_err = "dojo_comm_info: bad argument"; return DOJO_ERR_INVALID; }
    if (rank) *rank = s->comm_rank; if (world) *world = s->comm ? s->comm_world : 1;
    return DOJO_OK;
}

int dojo_set_gradient_mode(DojoHandle s, int32_t mode) {
    Enter enter_(s);
    if (!s || (mode != DOJO_GRAD_REFERENCE && mode != DOJO_GRAD_CONSISTENT)) { g_err = "dojo_set_gradient_mode: bad argument"; return DOJO_ERR_INVALID; }
    s->grad_mode = mode; return DOJO_OK;
}

int dojo_step_dev(DojoHandle s, const void* z, const void* u, void* z_next, int32_t* status, int32_t* iters, void* dz, void* du, void* stream) {
    Enter enter_(s);
    if (!s || !z || !z_next) { g_err = "dojo_step_dev: bad argument"; return DOJO_ERR_INVALID; }
    if ((dz == nullptr) != (du == nullptr) && s->M.nu > 0) { g_err = "dojo_step_dev: dz and du must both be given or both be NULL"; return DOJO_ERR_INVALID; }
    HIPCHK(hipSetDevice(s->device));
    size_t B = s->B, w = s->w;
    ENSURE(s->d_vel, B * 6 * s->M.Nb * w); ENSURE(s->d_jimp, B * (s->M.n_joint_imp + 1) * w);
    ENSURE(s->d_csg, B * (csg_per(s) * s->M.Nc + 1) * w);
    ENSURE(s->d_mu, B * sizeof(double));
    TRY(refuse_unsupported(s, dz != nullptr, false));
    const StepIO io{z, u, z_next, status, iters, dz, du, nullptr, nullptr};
    hipStream_t st = (hipStream_t)stream;
    const size_t NG = group_count(s, true, true);
    // Iteration cap (dojo_set_iteration_cap): in force for steps that are joined into the caller's stream -- there the step waits for its longest
    // solve.  An asynchronous handle chains its groups' steps without a barrier and hides that tail behind the other groups' kernels.
    const bool capped = !s->async && effective_cap(s) > 0;
    if (capped) {
        TRY(join_groups(s, st));                  // (asynchronous steps still in flight)
        TRY(begin_capped_step(s, std::max<size_t>(NG, 1), st));
    }
    const int rc = NG <= 1 ? step_single(s, io, st, capped) : capped ? step_capped_groups(s, io, st, NG) : step_plain_groups(s, io, st, NG);
    if (rc == DOJO_OK) s->have_solution = true;
    return rc;
}

// dojo_set_async(h, 1): dojo_step_dev no longer makes the caller's stream wait for the environment groups, so that
// consecutive steps of one group never wait for another group's straggler; dojo_join(h, stream) orders `stream` behind
// everything in flight (every host-pointer entry point does that implicitly).  dojo_set_groups: number of environment
// groups of dojo_step_dev (0 / negative: chosen from the batch size; 1: a single launch on the caller's stream).
int dojo_set_async(DojoHandle s, int32_t on) {
    Enter enter_(s);
    if (!s) { g_err = "dojo_set_async: bad argument"; return DOJO_ERR_INVALID; }
    s->async = on == 2 ? 2 : (on != 0 ? 1 : 0); return DOJO_OK;
}
// Order in which the step kernel's workgroups are handed to the GPU (no counterpart in the reference): 0 = batch order; 1 (default) = the longest
// solves of the previous step first, where that can matter -- steps joined into the caller's stream whose launch has more workgroups than the GPU
// holds at once: the launch ends with its last wavefront, and a 50-iteration solve that starts in the last round is that wavefront; 2 = always.
// Results do not depend on it.
int dojo_set_dispatch_order(DojoHandle s, int32_t mode) {
    Enter en_(s);
    if (!s || mode < 0 || mode > 2) { g_err = "dojo_set_dispatch_order: bad argument"; return DOJO_ERR_INVALID; }
    s->dispatch_mode = mode; return DOJO_OK;
}
int dojo_set_iteration_cap(DojoHandle s, int32_t cap) {
    Enter en_(s);
    if (!s) { g_err = "dojo_set_iteration_cap: bad argument"; return DOJO_ERR_INVALID; }
    s->iter_cap = cap <= 0 ? 0 : cap; return DOJO_OK;      // (0 or < 0: an EXPLICIT off -- DOJO_ITER_CAP in the environment only decides for handles that never called this)
}
int dojo_set_groups(DojoHandle s, int32_t n) {
    Enter enter_(s);
    if (!s) { g_err = "dojo_set_groups: bad argument"; return DOJO_ERR_INVALID; }
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipDeviceSynchronize());
    s->pending = false; s->groups = n > 0 ? n : -1; return DOJO_OK;
}
int dojo_join(DojoHandle s, void* stream) {
    Enter enter_(s);
    if (!s) { g_err = "dojo_join: bad argument"; return DOJO_ERR_INVALID; }
    HIPCHK(hipSetDevice(s->device));
    return join_groups(s, (hipStream_t)stream);
}

int dojo_step(DojoHandle s, const void* z, const void* u, void* z_next, int32_t* status, int32_t* iters, int32_t with_gradient) {
    Enter enter_(s);
    if (!s || !z || !z_next) { g_err = "dojo_step: bad argument"; return DOJO_ERR_INVALID; }
    HIPCHK(hipSetDevice(s->device));
    size_t B = s->B, w = s->w, nz = 13 * s->M.Nb, nx = 12 * s->M.Nb, nu = s->M.nu;
    const void* d_u = nullptr;
    ENSURE(s->d_z, B * nz * w); ENSURE(s->d_zn, B * nz * w);
    if (with_gradient) { ENSURE(s->d_dz, B * nx * nx * w); ENSURE(s->d_du, B * nx * (nu + 1) * w); }
    TRY(upload_step(s, s->d_z, z, nz, u, &d_u));
    TRY(dojo_step_dev(s, s->d_z, d_u, s->d_zn, s->d_status, s->d_iters, with_gradient ? s->d_dz : nullptr, with_gradient ? s->d_du : nullptr, nullptr));
    TRY(download_step(s, z_next, s->d_zn, nz, status, iters));
    s->have_grad = with_gradient != 0; s->have_u = (u && nu);
    return DOJO_OK;
}

// The mehrotra!(mechanism) seam (src/solver/mehrotra.jl:9): at that point set_input!/input_impulse! (src/mechanism/set.jl:40-53,
// src/joints/*/input.jl) have already folded the controls into every body's state.JF2 / state.Jτ2 and cleared the joints'
// inputs, so the drop-in hands over body impulses, not u.  jf [B, 6Nb] = [JF2 (world frame); Jτ2 (body frame)] per body, as
// they enter the body residual (src/integrators/constraint.jl:20-21: d -= [JF2; Jτ2]).  They share the external-force slot:
// -Δt·[Fext; τext] and -[JF2; Jτ2] are the same term (constraint.jl:15-18), so the kernels read fext + jf/Δt.
int dojo_step_impulses(DojoHandle s, const void* z, const void* jf, void* z_next, int32_t* status, int32_t* iters) {
    Enter enter_(s);
    if (!s || !z || !jf || !z_next) { g_err = "dojo_step_impulses: bad argument"; return DOJO_ERR_INVALID; }
    HIPCHK(hipSetDevice(s->device));
    const size_t B = s->B, w = s->w, nz = 13 * s->M.Nb, nf = 6 * s->M.Nb;
    ENSURE(s->d_z, B * nz * w); ENSURE(s->d_zn, B * nz * w);
    ENSURE(s->d_jf, 2 * B * nf * w);               // [raw impulses | folded forces]
    HIPCHK(hipDeviceSynchronize());
    TRY(upload_step(s, s->d_z, z, nz));
    HIPCHK(hipMemcpy(s->d_jf, jf, B * nf * w, hipMemcpyHostToDevice));
    void* folded = (char*)s->d_jf + B * nf * w;
    TRY(by_dtype(s, [&](auto t) { return launch_fold_impulses<decltype(t)>(s, s->d_jf, folded, nullptr); }));
    const void* user_fext = s->fext;
    s->fext = folded;
    const int rc = dojo_step_dev(s, s->d_z, nullptr, s->d_zn, s->d_status, s->d_iters, nullptr, nullptr, nullptr);
    s->fext = user_fext;
    TRY(rc);
    TRY(download_step(s, z_next, s->d_zn, nz, status, iters));
    s->have_grad = false; s->have_u = false;
    return DOJO_OK;
}

int dojo_get_solution(DojoHandle s, void* vel, void* joint_imp, void* contact_sg) {
    Enter enter_(s);
    if (!s || !s->have_solution) { g_err = "dojo_get_solution: no step has been taken"; return DOJO_ERR_INVALID; }
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipDeviceSynchronize());
    size_t B = s->B, w = s->w;
    if (vel) HIPCHK(hipMemcpy(vel, s->d_vel, B * 6 * s->M.Nb * w, hipMemcpyDeviceToHost));
    if (joint_imp && s->M.n_joint_imp) HIPCHK(hipMemcpy(joint_imp, s->d_jimp, B * s->M.n_joint_imp * w, hipMemcpyDeviceToHost));
    if (contact_sg && s->M.Nc) HIPCHK(hipMemcpy(contact_sg, s->d_csg, B * csg_per(s) * s->M.Nc * w, hipMemcpyDeviceToHost));
    return DOJO_OK;
}

// which row of g_variants steps this handle: out = [family (the FAM_* order), MAXC, wavefronts per workgroup (0: lane mapping)].  Reads the tables only.
int dojo_get_kernel_build(DojoHandle s, int32_t out[3]) {
    if (!s || !out) { g_err = "dojo_get_kernel_build: bad argument"; return DOJO_ERR_INVALID; }
    const Variant* v = variant_of(s->M, mapping_waves(s->M));
    if (!v) { g_err = "dojo_get_kernel_build: no kernel build serves this mechanism"; return DOJO_ERR_UNSUPPORTED; }
    out[0] = v->family; out[1] = v->maxc; out[2] = v->waves;
    return DOJO_OK;
}

// mechanism.μ (the central-path parameter, src/solver/mehrotra.jl:45) of every environment when the last step's solve
// returned: what a mehrotra! drop-in writes back before it calls set_entries! to leave mechanism.system as the reference does
int dojo_get_mu(DojoHandle s, double* mu) {
    Enter enter_(s);
    if (!s || !mu || !s->have_solution || !s->d_mu) { g_err = "dojo_get_mu: no step has been taken"; return DOJO_ERR_INVALID; }
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(mu, s->d_mu, (size_t)s->B * sizeof(double), hipMemcpyDeviceToHost));
    return DOJO_OK;
}

// Diagnostics of the final linearization of every environment's last step (quad mappings), fp64 [B, 2]:
// [0] max γ/s over its cones (what dojo_set_refinement's threshold is compared with), [1] the largest multiplier of the
// un-pivoted Gauss-Jordan eliminations (growth: ~1 for a well-scaled step, >> 1e3 when a joint row repeats a stiff contact row).
// Switched on by the first call (the following steps record them).
int dojo_get_diagnostics(DojoHandle s, double* diag) {
    Enter enter_(s);
    if (!s) { g_err = "dojo_get_diagnostics: bad argument"; return DOJO_ERR_INVALID; }
    HIPCHK(hipSetDevice(s->device));
    if (!s->d_diag) {
        ENSURE(s->d_diag, (size_t)s->B * 2 * sizeof(double));
        HIPCHK(hipMemset(s->d_diag, 0, (size_t)s->B * 2 * sizeof(double)));
    }
    HIPCHK(hipDeviceSynchronize());
    if (diag) HIPCHK(hipMemcpy(diag, s->d_diag, (size_t)s->B * 2 * sizeof(double), hipMemcpyDeviceToHost));
    return DOJO_OK;
}

int dojo_gradients(DojoHandle s, void* dz, void* du) {
    Enter enter_(s);
    if (!s || !s->have_grad) { g_err = "dojo_gradients: the last dojo_step was not run with with_gradient=1"; return DOJO_ERR_INVALID; }
    HIPCHK(hipSetDevice(s->device));
    const size_t nx = 12 * s->M.Nb, nu = s->M.nu;      // host layout: [B, nx, nx] / [B, nx, nu] row-major
    if (dz) TRY(download_transposed(s, dz, s->d_dz, nx, nx));
    if (du && nu) TRY(download_transposed(s, du, s->d_du, nx, nu));
    return DOJO_OK;
}

// the handle's buffers a rollout uses, allocated on first use
static int ensure_rollout(DojoHandle s, const RolloutIO& io) {
    const size_t B = s->B, w = s->w, nz = 13 * s->M.Nb;
    ENSURE(s->d_z, B * nz * w); ENSURE(s->d_zn, B * nz * w);
    ENSURE(s->d_vel, B * 6 * s->M.Nb * w); ENSURE(s->d_jimp, B * (s->M.n_joint_imp + 1) * w);
    ENSURE(s->d_csg, B * (csg_per(s) * s->M.Nc + 1) * w);
    if (io.storage) ENSURE(s->d_res, B * 6 * s->M.Nb * w);
    if (io.controller && !io.U_out) ENSURE(s->d_pu, B * s->M.nu * w);
    if (io.A) {                                      // (the buffers of dojo_minimal_gradients_dev, sized as there)
        const size_t Nb = s->M.Nb, nx = 12 * Nb, nu = s->M.nu, nm = 2 * nu;
        ENSURE(s->d_dz, B * nx * nx * w); ENSURE(s->d_du, B * nx * (nu + 1) * w);
        ENSURE(s->d_jm, B * nx * (nm + 1) * sizeof(double)); ENSURE(s->d_jt, B * nx * (nm + 1) * sizeof(double));
        ENSURE(s->d_jb, B * Nb * 12 * 24 * sizeof(double));
    }
    return DOJO_OK;
}

// simulate! with pre-sampled controls (src/simulation/simulate.jl:16-37): H steps, each fed with the previous step's
// internal next state, and whatever of RolloutIO is asked for recorded along the way
static int rollout_core(DojoHandle s, int32_t H, const RolloutIO& io, void* stream) {
    if (!s || !io.z0 || H < 1) { g_err = "dojo_rollout_dev: bad argument"; return DOJO_ERR_INVALID; }
    HIPCHK(hipSetDevice(s->device));
    size_t B = s->B, w = s->w, nz = 13 * s->M.Nb, nu = s->M.nu, nx = 12 * s->M.Nb;
    TRY(ensure_rollout(s, io));
    const Controller* pol = io.controller;
    const size_t nobs = pol ? 2 * nu + (pol->contact_forces() ? (size_t)s->M.Nc : 0) : 0;
    auto at = [](void* p, size_t offset) -> char* { return p ? (char*)p + offset : nullptr; };      // step k of an array that is recorded
    // in minimal coordinates: the chain of dojo_minimal_gradients_dev for step k of a group into A[k], Bm[k], from the handle's d_dz, d_du that step has just written
    const bool minimal = pol && pol->tracking, literal = io.A && s->grad_mode == DOJO_GRAD_REFERENCE;
    auto minimal_chain = [&](int k, const Span& sp) {
        const size_t kB = (size_t)k * B, n = 2 * nu;
        const void* xj = at(io.OBS, (literal ? kB + B : kB) * n * w);                              // where the min -> max Jacobian is evaluated: X[k + 1] / X[k] ...
        const void* zj = literal ? (const void*)s->d_zn : (const void*)s->d_z;                     // ... and the maximal state that belongs to it
        return by_dtype(s, [&](auto t) { return launch_minimal_chain<decltype(t)>(s, sp, xj, zj, literal ? 1 : 0, at(io.A, kB * n * n * w), at(io.Bm, kB * n * nu * w)); });
    };
    hipStream_t st = (hipStream_t)stream;
    const char* cur = (const char*)io.z0;   // the state a group's next step starts from; behind the loops: the last state (the same buffer for every group)
    int slot = -1; TRY(begin_timing(s, &slot, st));
    // Environments are independent, so the batch is rolled out as NG groups on internal streams: a group whose step
    // contains an environment that runs into max_iter (one wavefront, ~5x the mean step time) delays only itself while
    // the other groups' launches keep the GPU busy.  (ROCm runs at most GPU_MAX_HW_QUEUES streams concurrently.)
    TRY(join_groups(s, st));                  // (asynchronous steps still in flight)
    // With A, Bm the batch is one group on the caller's stream: min2max_jac_kernel keeps 8.9 KB of scratch per lane, and ROCr sizes a hardware queue's scratch for a
    // full GPU of such wavefronts -- on the groups' internal queues as well that ends in HSA_STATUS_ERROR_OUT_OF_RESOURCES (group_count has the same rule for the
    // builds with large scratch).  The chain then runs where dojo_minimal_gradients_dev runs it: one queue's worth of scratch.
    const size_t NG = io.A ? 1 : group_count(s, H >= 2);
    const Partition P(B, NG);
    const Mode m = step_mode(s, NG, false, true);
    ForkGuard guard{s, st, NG > 1};
    if (NG > 1) { TRY(ensure_groups(s, NG)); HIPCHK(hipEventRecord(s->fork_event, st)); }
    for (size_t gi = 0; gi < P.groups(); ++gi) {
        const Span sp = P.span(gi, NG > 1 ? s->gstreams[gi] : st);
        if (NG > 1) HIPCHK(hipStreamWaitEvent(sp.stream, s->fork_event, 0));
        cur = (const char*)io.z0;
        for (int k = 0; k < H; ++k) {
            const size_t kB = (size_t)k * B;
            char* nxt = io.Z ? at(io.Z, kB * nz * w) : (char*)((minimal || !(k & 1)) ? s->d_zn : s->d_z);
            const char* uk = nu ? at((void*)io.U, kB * nu * w) : nullptr;
            if (pol) {
                char* upol = io.U_out ? at(io.U_out, kB * nu * w) : (char*)s->d_pu;
                TRY(launch_controller(s, *pol, k, cur, (k > 0 || pol->contact_init()) ? s->d_csg : nullptr, uk, at(io.OBS, kB * nobs * w), upol, sp, minimal ? s->d_z : nullptr));
                uk = upol;
                if (minimal) cur = (const char*)s->d_z;      // the step starts from the re-projected X[k]
            }
            // DOJO_GRAD_REFERENCE evaluates the chain of step k - 1 at X[k], which that controller has just written, and at the state step k - 1 left: in front of step k, which overwrites it
            if (literal && k > 0) TRY(minimal_chain(k - 1, sp));
            int32_t* stk = io.status ? io.status + kB : nullptr;
            void* const dzk = io.A ? s->d_dz : at(io.DZ, kB * nx * nx * w); void* const duk = io.A ? s->d_du : nu ? at(io.DU, kB * nx * nu * w) : nullptr;
            TRY(launch_any(s, StepIO{cur, uk, nxt, stk, nullptr, dzk, duk, nullptr, at(io.storage, kB * 25 * s->M.Nb * w)}, sp, m));
            // (the same Mode: the same hand-off record, no timing slot -- m.slot is null --, and a launch with io.dc never reorders the dispatch)
            if (io.DC && s->M.Nc > 0) TRY(launch_any(s, StepIO{cur, uk, nxt, nullptr, nullptr, nullptr, nullptr, at(io.DC, kB * nx * 5 * s->M.Nc * w), nullptr}, sp, m));
            // DOJO_GRAD_CONSISTENT evaluates it at X[k] and the step's input: behind the step, in front of the next controller, which overwrites that input
            if (io.A && !literal) TRY(minimal_chain(k, sp));
            cur = nxt;
        }
        if (pol && io.OBS) TRY(launch_controller(s, *pol, H, cur, s->d_csg, nullptr, at(io.OBS, (size_t)H * B * nobs * w), nullptr, sp));      // the observation of the final state
        if (literal) TRY(minimal_chain(H - 1, sp));
        if (NG > 1) { HIPCHK(hipEventRecord(s->gevents[gi], sp.stream)); HIPCHK(hipStreamWaitEvent(st, s->gevents[gi], 0)); }
    }
    TRY(end_timing(s, slot, false, H, st));
    if (!io.Z && cur != (const char*)s->d_zn) HIPCHK(hipMemcpyAsync(s->d_zn, cur, B * nz * w, hipMemcpyDeviceToDevice, st));
    s->have_solution = true; s->have_grad = false;
    return guard.done();
}

// what a recording entry refuses on top of its own checks: refuse_unsupported's text, with the entry point in front of it
static int refuse_record(DojoHandle s, const char* who, bool want_dc = false) {
    const int rc = refuse_unsupported(s, true, want_dc);
    if (rc != DOJO_OK) g_err = std::string(who) + ": " + g_err.c_str();
    return rc;
}

// What the reverse sweeps (*_adjoint_dev) refuse alike, in the order they refuse it: the horizon, the entry's required arrays, the cotangent space, the entry's
// further conditions, the alignment of the two Jacobian arrays the kernel reads (J1: null when it reads one)
struct Refusal { bool applies; const char* text; };
static int refuse_sweep(const char* who, int32_t H, std::initializer_list<Refusal> required, int32_t cot_space, const void* Z, std::initializer_list<Refusal> further,
                        const void* J0, const void* J1, const char* jacobians) {
    const std::string w_ = std::string(who) + ": ";
    if (H < 1) { g_err = w_ + "H must be >= 1"; return DOJO_ERR_INVALID; }
    for (const Refusal& r : required) if (r.applies) { g_err = w_ + r.text; return DOJO_ERR_INVALID; }
    if (cot_space != 0 && cot_space != 1) { g_err = w_ + "cot_space must be 0 (tangent) or 1 (state)"; return DOJO_ERR_INVALID; }
    if (cot_space == 1 && !Z) { g_err = w_ + "cot_space = 1 needs the states Z"; return DOJO_ERR_INVALID; }
    for (const Refusal& r : further) if (r.applies) { g_err = w_ + r.text; return DOJO_ERR_INVALID; }
    if (((uintptr_t)J0 | (uintptr_t)J1) & 15) { g_err = w_ + jacobians + " must be 16-byte aligned (the kernel reads them in 16-byte pieces)"; return DOJO_ERR_INVALID; }
    return DOJO_OK;
}

// The memory refusal of the *_gradients host entries, before anything is read, allocated or launched: what the call is going to allocate -- its staging buffers and
// what `handle` measured of the handle's workspaces -- against the free device memory.  `what` opens the text, up to the byte count of the need.
static int refuse_memory(const std::string& what, const Staging& st, const Measuring& handle, const char* verb) {
    const size_t need = st.bytes() + handle.bytes;
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    if (need <= free_b) return DOJO_OK;
    g_err = what + std::to_string(need) + " bytes with the other buffers of the call) " + verb + " not fit into the " + std::to_string(free_b) + " bytes of free device memory";
    return DOJO_ERR_INVALID;
}
// the workspaces a recording rollout takes on first use: those of rollout_core (the recording host entries keep no storage and record U_out: the io-dependent buffers of
// ensure_rollout are not theirs) and of its differentiable step launches (sized for the whole batch, so one group's geometry gives them all)
static int ensure_record(DojoHandle s) {
    TRY(ensure_rollout(s, RolloutIO{}));
    return ensure_workspaces(s, StepIO{}, step_mode(s, 1, false, true), geometry_of(s, whole_batch(s, nullptr), true), true, false);
}

int dojo_rollout_dev(DojoHandle s, const void* z0, const void* U, int32_t H, void* Z, int32_t* status, void* stream) {
    Enter enter_(s);
    RolloutIO io; io.z0 = z0; io.U = U; io.Z = Z; io.status = status;
    return rollout_core(s, H, io, stream);
}

int dojo_simulate_dev(DojoHandle s, const void* z0, const void* U, int32_t H, void* Z, void* storage, int32_t* status, void* stream) {
    Enter enter_(s);
    if (!storage) { g_err = "dojo_simulate_dev: storage must not be NULL (use dojo_rollout_dev for record = false)"; return DOJO_ERR_INVALID; }
    RolloutIO io; io.z0 = z0; io.U = U; io.Z = Z; io.status = status; io.storage = storage;
    return rollout_core(s, H, io, stream);
}

// dojo_rollout_dev plus the IFT Jacobians of every step, left on the device for dojo_rollout_adjoint_dev
int dojo_rollout_record_dev(DojoHandle s, const void* z0, const void* U, int32_t H, void* Z, int32_t* status, void* DZ, void* DU, void* stream) {
    Enter enter_(s);
    if (!s || !z0 || H < 1 || !Z || !DZ || (!DU && s->M.nu > 0)) { g_err = "dojo_rollout_record_dev: bad argument (z0, Z, DZ and -- with nu > 0 -- DU are required, H >= 1)"; return DOJO_ERR_INVALID; }
    TRY(refuse_unsupported(s, true, false));
    RolloutIO io; io.z0 = z0; io.U = U; io.Z = Z; io.status = status; io.DZ = DZ; io.DU = DU;
    return rollout_core(s, H, io, stream);
}

// Closed-loop rollouts: what is refused, before anything is launched or allocated
static int refuse_policy(DojoHandle s, const void* z0, const DojoPolicy* p, int32_t H, const char* who) {
    const std::string w_ = std::string(who) + ": ";
    if (!s || !z0 || !p || !p->W) { g_err = w_ + "bad argument (handle, z0, policy and policy->W are required)"; return DOJO_ERR_INVALID; }
    if (H < 1) { g_err = w_ + "H must be >= 1"; return DOJO_ERR_INVALID; }
    if (s->M.nu == 0) { g_err = w_ + "the mechanism has no inputs"; return DOJO_ERR_INVALID; }
    if (p->na < 1 || p->act_off < 0 || (long long)p->act_off + p->na > (long long)s->M.nu) { g_err = w_ + "the policy must drive inputs act_off .. act_off + na - 1 inside 0 .. nu - 1, na >= 1"; return DOJO_ERR_INVALID; }
    if (p->contact_init && !s->have_solution) { g_err = w_ + "contact_init = 1 needs a step on this handle"; return DOJO_ERR_INVALID; }
    TRY(refuse_minimal(s, who));
    if (p->contact_forces && s->M.contact_model == 2) { g_err = w_ + "contact forces are not available for LinearContact mechanisms"; return DOJO_ERR_UNSUPPORTED; }
    if (dj::policy::lds_bytes(2 * s->M.nu + s->M.Nc) > 65536) { g_err = w_ + "supports at most 2048 observations per environment (they are kept in LDS)"; return DOJO_ERR_UNSUPPORTED; }
    return DOJO_OK;
}

int dojo_rollout_policy_dev(DojoHandle s, const void* z0, const DojoPolicy* policy, int32_t H, void* Z, void* OBS, void* U_out, int32_t* status, void* stream) {
    Enter enter_(s);
    TRY(refuse_policy(s, z0, policy, H, "dojo_rollout_policy_dev"));
    const DojoPolicy p = *policy;      // (the caller's struct is read during the call only)
    Controller c; c.affine = &p;
    RolloutIO io; io.z0 = z0; io.U = p.U_ff; io.Z = Z; io.status = status; io.controller = &c; io.OBS = OBS; io.U_out = U_out;
    return rollout_core(s, H, io, stream);
}

// host pointers (the members of *policy too): upload, roll out on the device, download
int dojo_rollout_policy(DojoHandle s, const void* z0, const DojoPolicy* policy, int32_t H, void* Z, void* OBS, void* U_out, int32_t* status) {
    Enter enter_(s);
    TRY(refuse_policy(s, z0, policy, H, "dojo_rollout_policy"));
    HIPCHK(hipSetDevice(s->device));
    const size_t B = s->B, w = s->w, nz = 13 * s->M.Nb, nu = s->M.nu, HB = (size_t)H * B, na = (size_t)policy->na, Bw = policy->per_env ? B : 1;
    const size_t nobs = 2 * nu + (policy->contact_forces ? (size_t)s->M.Nc : 0);
    Staging st;
    const auto &dz0 = st.input(B * nz * w, z0), &dW = st.input(Bw * na * nobs * w, policy->W), &db = st.input(Bw * na * w, policy->bias);
    const auto &dm = st.input(nobs * w, policy->mean), &dsc = st.input(nobs * w, policy->scale), &dUff = st.input(HB * nu * w, policy->U_ff);
    const auto &dZ = st.output(HB * nz * w, Z), &dO = st.output((HB + B) * nobs * w, OBS), &dU = st.output(HB * nu * w, U_out), &dS = st.output(HB * sizeof(int), status);
    TRY(st.allocate());
    DojoPolicy p = *policy; p.W = dW.p; p.bias = db.p; p.mean = dm.p; p.scale = dsc.p; p.U_ff = dUff.p;
    Controller c; c.affine = &p;
    RolloutIO io; io.z0 = dz0.p; io.U = p.U_ff; io.Z = dZ.p; io.status = (int32_t*)dS.p; io.controller = &c; io.OBS = dO.p; io.U_out = dU.p;
    TRY(rollout_core(s, H, io, nullptr));
    return st.finish(s, dZ, H);
}

int dojo_rollout_adjoint_dev(DojoHandle s, int32_t H, const void* DZ, const void* DU, const void* G, int32_t cot_space, const void* Z, const int32_t* status,
                             void* gU, void* gz, void* stream) {
    Enter enter_(s);
    const char* who = "dojo_rollout_adjoint_dev";
    if (!s) { g_err = std::string(who) + ": bad argument"; return DOJO_ERR_INVALID; }
    if (s->M.nu == 0) gU = nullptr;
    TRY(refuse_sweep(who, H, {{!DZ || !G, "DZ and G must not be NULL"}}, cot_space, Z, {{gU && !DU, "gU needs DU"}}, DZ, gU ? DU : nullptr, "DZ and DU"));
    if (dj::adjoint::lds_bytes(12 * s->M.Nb) > 65536) { g_err = std::string(who) + ": supports at most 170 bodies (lambda is kept in LDS)"; return DOJO_ERR_UNSUPPORTED; }
    HIPCHK(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    TRY(join_groups(s, st));                  // (asynchronous steps still in flight: they may be writing the Jacobians)
    if (!gU && !gz) return DOJO_OK;
    return by_dtype(s, [&](auto t) { return launch_adjoint<decltype(t)>(s, H, DZ, DU, G, cot_space, Z, status, gU, gz, st); });
}

// host pointers: upload, record on the device, reverse sweep, download -- the Jacobians never cross PCIe
int dojo_rollout_gradients(DojoHandle s, const void* z0, const void* U, int32_t H, const void* G, int32_t cot_space, void* Z, int32_t* status, void* gU, void* gz) {
    Enter enter_(s);
    const std::string who = "dojo_rollout_gradients";
    if (!s || !z0 || !G || H < 1 || (cot_space != 0 && cot_space != 1)) { g_err = who + ": bad argument"; return DOJO_ERR_INVALID; }
    TRY(refuse_unsupported(s, true, false));
    HIPCHK(hipSetDevice(s->device));
    const size_t B = s->B, w = s->w, nz = 13 * s->M.Nb, nx = 12 * s->M.Nb, nu = s->M.nu, HB = (size_t)H * B, ng = cot_space ? nz : nx;
    Staging st;
    const auto &dz0 = st.input(B * nz * w, z0), &dG = st.input(HB * ng * w, G), &dU = st.input(HB * nu * w, nu ? U : nullptr);
    const auto &dZ = st.kept(HB * nz * w, Z), &dS = st.kept(HB * sizeof(int), status), &dDZ = st.kept(HB * nx * nx * w), &dDU = st.kept(HB * nx * nu * w);
    const auto &dgU = st.kept(HB * nu * w, nu ? gU : nullptr), &dgz = st.kept(B * nx * w, gz);
    {
        Measuring handle(s);
        TRY(ensure_record(s));
        TRY(refuse_memory(who + ": the record of " + std::to_string(HB * nx * (nx + nu) * w) + " bytes (H B nx (nx + nu) scalars; ", st, handle, "does"));
    }
    TRY(st.allocate());
    RolloutIO io; io.z0 = dz0.p; io.U = dU.p; io.Z = dZ.p; io.status = (int32_t*)dS.p; io.DZ = dDZ.p; io.DU = dDU.p;
    TRY(rollout_core(s, H, io, nullptr));
    TRY(dojo_rollout_adjoint_dev(s, H, dDZ.p, dDU.p, dG.p, cot_space, dZ.p, (const int32_t*)dS.p, dgU.p, dgz.p, nullptr));
    return st.finish(s, dZ, H);
}

// ---- contact-data gradients through rollouts (dojo_data_adjoint.hpp): get_contact_gradients (src/gradients/contact.jl:1-55) per step, chained as in
// examples/system_identification/utilities.jl:42-90, in reverse mode on the device ----
// dojo_rollout_record_dev plus the contact-data columns of every step, DC [H][B][5Nc][nx] in the layout of dojo_contact_gradients_dev
int dojo_rollout_data_record_dev(DojoHandle s, const void* z0, const void* U, int32_t H, void* Z, int32_t* status, void* DZ, void* DU, void* DC, void* stream) {
    if (!DC) return dojo_rollout_record_dev(s, z0, U, H, Z, status, DZ, DU, stream);
    Enter enter_(s);
    const char* who = "dojo_rollout_data_record_dev";
    if (!s || !z0 || H < 1 || !Z || !DZ || (!DU && s->M.nu > 0)) { g_err = std::string(who) + ": bad argument (z0, Z, DZ and -- with nu > 0 -- DU are required, H >= 1)"; return DOJO_ERR_INVALID; }
    // body-body contacts, Impact / Linear contacts, more than 64 contacts, the lane mapping: refused before anything is allocated or launched
    TRY(refuse_record(s, who, s->M.Nc > 0));
    RolloutIO io; io.z0 = z0; io.U = U; io.Z = Z; io.status = status; io.DZ = DZ; io.DU = DU; io.DC = DC;
    return rollout_core(s, H, io, stream);
}

int dojo_rollout_data_adjoint_dev(DojoHandle s, int32_t H, const void* DZ, const void* DC, const void* G, int32_t cot_space, const void* Z, const int32_t* status,
                                  void* gtheta_env, void* gtheta, void* gz, void* stream) {
    Enter enter_(s);
    const char* who = "dojo_rollout_data_adjoint_dev";
    if (!s) { g_err = std::string(who) + ": bad argument"; return DOJO_ERR_INVALID; }
    const int Nc = s->M.Nc;
    TRY(refuse_sweep(who, H, {{!DZ || !G, "DZ and G must not be NULL"}, {!DC && Nc > 0, "DC must not be NULL (a mechanism without contacts has none)"}}, cot_space, Z,
                     {{!gtheta_env && !gtheta && !gz, "gtheta_env, gtheta and gz are all NULL"}}, DZ, Nc > 0 ? DC : nullptr, "DZ and DC"));
    if (dj::dadjoint::lds_bytes(12 * s->M.Nb, 5 * Nc) > 65536) { g_err = std::string(who) + ": lambda, g and the 5 Nc accumulators (4 nx + 5 Nc doubles) do not fit into 64 KB of LDS"; return DOJO_ERR_UNSUPPORTED; }
    if (Nc == 0) { gtheta_env = nullptr; gtheta = nullptr; }      // no contact data: gz alone, the gtheta outputs are not touched
    HIPCHK(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    TRY(join_groups(s, st));                  // (asynchronous steps still in flight: they may be writing the Jacobians)
    if (!gtheta_env && !gtheta && !gz) return DOJO_OK;
    if (gtheta) TRY(ensure_dacc(s));
    double* acc = gtheta ? s->d_dacc : nullptr;
    return by_dtype(s, [&](auto t) { return launch_data_adjoint<decltype(t)>(s, H, DZ, DC, G, cot_space, Z, status, gtheta_env, acc, gtheta, gz, st); });
}

// host pointers: upload, record on the device (with the contact-data columns), the contact-data sweep -- and the open-loop sweep over the same record when gU is
// wanted --, download.  The Jacobians never cross PCIe.
int dojo_rollout_data_gradients(DojoHandle s, const void* z0, const void* U, int32_t H, const void* G, int32_t cot_space, void* Z, int32_t* status,
                                void* gtheta, void* gtheta_env, void* gU, void* gz) {
    Enter enter_(s);
    const std::string who = "dojo_rollout_data_gradients";
    if (!s || !z0 || !G || H < 1 || (cot_space != 0 && cot_space != 1)) { g_err = who + ": bad argument"; return DOJO_ERR_INVALID; }
    TRY(refuse_record(s, who.c_str(), s->M.Nc > 0));
    HIPCHK(hipSetDevice(s->device));
    const size_t B = s->B, w = s->w, nz = 13 * s->M.Nb, nx = 12 * s->M.Nb, nu = s->M.nu, nth = 5 * (size_t)s->M.Nc, HB = (size_t)H * B, ng = cot_space ? nz : nx;
    if (!nth) { gtheta = nullptr; gtheta_env = nullptr; }      // no contact data: these outputs are not touched
    Staging st;
    const auto &dz0 = st.input(B * nz * w, z0), &dG = st.input(HB * ng * w, G), &dU = st.input(HB * nu * w, nu ? U : nullptr);
    const auto &dZ = st.kept(HB * nz * w, Z), &dS = st.kept(HB * sizeof(int), status);
    const auto &dDZ = st.kept(HB * nx * nx * w), &dDU = st.kept(HB * nx * nu * w), &dDC = st.kept(HB * nx * nth * w);
    const auto &dgt = st.kept(nth * w, gtheta), &dgte = st.kept(B * nth * w, gtheta_env), &dgU = st.kept(HB * nu * w, nu ? gU : nullptr), &dgz = st.kept(B * nx * w, gz);
    {
        Measuring handle(s);
        TRY(ensure_record(s));
        if (gtheta) TRY(ensure_dacc(s));
        TRY(refuse_memory(who + ": the record of " + std::to_string(HB * nx * (nx + nu + nth) * w) + " bytes (H B nx (nx + nu + 5 Nc) scalars; ", st, handle, "does"));
    }
    TRY(st.allocate());
    RolloutIO io; io.z0 = dz0.p; io.U = dU.p; io.Z = dZ.p; io.status = (int32_t*)dS.p; io.DZ = dDZ.p; io.DU = dDU.p; io.DC = dDC.p;
    TRY(rollout_core(s, H, io, nullptr));
    TRY(dojo_rollout_data_adjoint_dev(s, H, dDZ.p, dDC.p, dG.p, cot_space, dZ.p, (const int32_t*)dS.p, gtheta_env ? dgte.p : nullptr, gtheta ? dgt.p : nullptr, dgz.p, nullptr));
    if (gU && nu) TRY(dojo_rollout_adjoint_dev(s, H, dDZ.p, dDU.p, dG.p, cot_space, dZ.p, (const int32_t*)dS.p, dgU.p, nullptr, nullptr));
    return st.finish(s, dZ, H);
}

// ---- forward mode over the same records (dojo_tangent.hpp): T tangent directions in one pass, the chain of examples/system_identification/utilities.jl:42-90 ----
int dojo_rollout_tangent_dev(DojoHandle s, int32_t H, int32_t T, const void* DZ, const void* DU, const void* DC, const void* dz0, const void* dU, const void* dtheta,
                             int32_t tan_space, const void* Z, const int32_t* status, void* dZ, void* stream) {
    Enter enter_(s);
    const char* who = "dojo_rollout_tangent_dev";
    if (!s) { g_err = std::string(who) + ": bad argument"; return DOJO_ERR_INVALID; }
    const int nx = 12 * s->M.Nb, nu = (int)s->M.nu, nth = 5 * s->M.Nc;
    if (nu == 0) dU = nullptr;
    if (nth == 0) dtheta = nullptr;
    // (the space of the output is this entry's own argument: refuse_sweep's cot_space rule is given nothing to object to, the two tan_space rules are `further` ones;
    //  its second Jacobian pointer carries the low bits of both DU and DC, which is all the alignment rule looks at)
    TRY(refuse_sweep(who, H, {{T < 1, "T must be >= 1"}, {!DZ || !dZ, "DZ and dZ must not be NULL"},
                              {!dz0 && !dU && !dtheta, "dz0, dU and dtheta are all NULL (or ignored: dU with nu = 0, dtheta with Nc = 0)"}}, 0, nullptr,
                     {{dU && !DU, "dU needs DU"}, {dtheta && !DC, "dtheta needs DC"}, {tan_space != 0 && tan_space != 1, "tan_space must be 0 (tangent) or 1 (state)"},
                      {tan_space == 1 && !Z, "tan_space = 1 needs the states Z"}},
                     DZ, (const void*)((uintptr_t)(dU ? DU : nullptr) | (uintptr_t)(dtheta ? DC : nullptr)), "DZ, DU and DC"));
    if (!dj::tangent::fits(nx, s->w) || dj::tangent::lds_bytes(nx, nu, nth, s->w) > 65536) {
        g_err = std::string(who) + ": a column of 16-byte pieces must fit a workgroup's 256 lanes (nx <= 512 in fp64, 1024 in fp32) and the step's inputs and partial sums into 64 KB of LDS";
        return DOJO_ERR_UNSUPPORTED;
    }
    HIPCHK(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    TRY(join_groups(s, st));                  // (asynchronous steps still in flight: they may be writing the Jacobians)
    return by_dtype(s, [&](auto t) { return launch_tangent<decltype(t)>(s, H, T, DZ, DU, DC, dz0, dU, dtheta, tan_space, Z, status, dZ, st); });
}

// host pointers: upload, record on the device (DU only for dU, DC only for dtheta), forward sweep, download -- the Jacobians never cross PCIe
int dojo_rollout_tangents(DojoHandle s, const void* z0, const void* U, int32_t H, int32_t T, const void* dz0, const void* dU, const void* dtheta, int32_t tan_space,
                          void* Z, int32_t* status, void* dZ) {
    Enter enter_(s);
    const std::string who = "dojo_rollout_tangents";
    if (!s || !z0 || !dZ || H < 1 || T < 1 || (tan_space != 0 && tan_space != 1)) { g_err = who + ": bad argument (z0 and dZ are required, H >= 1, T >= 1, tan_space 0 or 1)"; return DOJO_ERR_INVALID; }
    const size_t B = s->B, w = s->w, nz = 13 * s->M.Nb, nx = 12 * s->M.Nb, nu = s->M.nu, nth = 5 * (size_t)s->M.Nc, HB = (size_t)H * B, nout = tan_space ? nz : nx;
    if (!nu) dU = nullptr;
    if (!nth) dtheta = nullptr;
    if (!dz0 && !dU && !dtheta) { g_err = who + ": dz0, dU and dtheta are all NULL (or ignored: dU with nu = 0, dtheta with Nc = 0)"; return DOJO_ERR_INVALID; }
    TRY(refuse_record(s, who.c_str(), dtheta != nullptr));
    HIPCHK(hipSetDevice(s->device));
    Staging st;
    const auto &dz = st.input(B * nz * w, z0), &dUc = st.input(HB * nu * w, nu ? U : nullptr);
    const auto &ddz0 = st.input(B * T * nx * w, dz0), &ddU = st.input(HB * T * nu * w, dU), &ddth = st.input((size_t)T * nth * w, dtheta);
    const auto &dZs = st.kept(HB * nz * w, Z), &dS = st.kept(HB * sizeof(int), status);
    const auto &dDZ = st.kept(HB * nx * nx * w), &dDU = st.kept(HB * nx * nu * w, nullptr, dU != nullptr), &dDC = st.kept(HB * nx * nth * w, nullptr, dtheta != nullptr);
    const auto &ddZ = st.kept(HB * T * nout * w, dZ);
    {
        Measuring handle(s);
        TRY(ensure_record(s));
        TRY(refuse_memory(who + ": the record of " + std::to_string(HB * nx * (nx + (dU ? nu : 0) + (dtheta ? nth : 0)) * w) + " bytes (H B nx (nx + nu + 5 Nc) scalars, DU and DC as far as dU and dtheta ask for them; ",
                          st, handle, "does"));
    }
    TRY(st.allocate());
    RolloutIO io; io.z0 = dz.p; io.U = dUc.p; io.Z = dZs.p; io.status = (int32_t*)dS.p; io.DZ = dDZ.p; io.DU = dDU.p; io.DC = dDC.p;
    TRY(rollout_core(s, H, io, nullptr));
    TRY(dojo_rollout_tangent_dev(s, H, T, dDZ.p, dDU.p, dDC.p, ddz0.p, ddU.p, ddth.p, tan_space, dZs.p, (const int32_t*)dS.p, ddZ.p, nullptr));
    return st.finish(s, dZs, H);
}

// ---- batched iLQR: the Riccati backward pass in minimal coordinates (dojo_riccati.hpp), IterativeLQR's backward pass over get_minimal_gradients! ----
// what both entries refuse, before anything is allocated or launched
static int refuse_riccati(DojoHandle s, int32_t H, const DojoRiccati* r, const char* who) {
    const std::string w_ = std::string(who) + ": ";
    if (!s || !r) { g_err = w_ + "bad argument (the handle and the DojoRiccati record are required)"; return DOJO_ERR_INVALID; }
    if (H < 1) { g_err = w_ + "H must be >= 1"; return DOJO_ERR_INVALID; }
    if (!r->A || !r->Bm || !r->lx || !r->lu || !r->lxx || !r->luu || !r->K || !r->kff || !r->fail) {
        g_err = w_ + "A, Bm, lx, lu, lxx, luu, K, kff and fail must not be NULL"; return DOJO_ERR_INVALID;
    }
    if (s->M.nu == 0) { g_err = w_ + "the mechanism has no inputs"; return DOJO_ERR_INVALID; }
    if (r->na < 1 || r->act_off < 0 || (long long)r->act_off + r->na > (long long)s->M.nu) { g_err = w_ + "the policy must drive inputs act_off .. act_off + na - 1 inside 0 .. nu - 1, na >= 1"; return DOJO_ERR_INVALID; }
    TRY(refuse_minimal(s, who));
    const int n = 2 * (int)s->M.nu, m = r->na;
    const size_t lds = dj::riccati::lds_bytes(n, m);
    if (lds > 65536 || !dj::riccati::accumulators(n, m) || m > dj::riccati::MAX_M) {
        g_err = w_ + "n = " + std::to_string(n) + ", na = " + std::to_string(m) + " needs " + std::to_string(lds) + " bytes of LDS per environment; the kernel holds at most 65536, n + na <= 110 (the accumulators of [Qxx Qxu; Qux Quu] are registers) and na <= " + std::to_string(dj::riccati::MAX_M);
        return DOJO_ERR_UNSUPPORTED;
    }
    return DOJO_OK;
}

// ... and what the control-limited entries refuse on top (include/dojo_hip_limits.h)
static int refuse_riccati_box(DojoHandle s, int32_t H, const DojoRiccati* r, const RiccatiBox& box, const char* who) {
    TRY(refuse_riccati(s, H, r, who));
    const std::string w_ = std::string(who) + ": ";
    if (!box.lim || !box.U) { g_err = w_ + "lim and U must not be NULL"; return DOJO_ERR_INVALID; }
    const int n = 2 * (int)s->M.nu, m = r->na;
    const size_t lds = dj::riccati::box_lds_bytes(n, m);
    if (lds > 65536) {
        g_err = w_ + "n = " + std::to_string(n) + ", na = " + std::to_string(m) + " needs " + std::to_string(lds) + " bytes of LDS per environment with the box QP; the kernel holds at most 65536";
        return DOJO_ERR_UNSUPPORTED;
    }
    return DOJO_OK;
}
// the limits of a host entry are read: an empty interval or a NaN is refused (the device entries cannot look: there it is the failure code -(k + 1), or the law's comparison)
static int refuse_limit_values(DojoHandle s, const DojoControlLimits* lim, size_t count, const char* who) {
    return by_dtype(s, [&](auto t) {
        using T = decltype(t);
        const T* const lo = (const T*)lim->lo; const T* const hi = (const T*)lim->hi;
        for (size_t i = 0; i < count; ++i) {
            const double l = lo ? (double)lo[i] : -HUGE_VAL, h = hi ? (double)hi[i] : HUGE_VAL;
            if (!(l <= h)) { g_err = std::string(who) + ": the limits must satisfy lo <= hi and must not be NaN (element " + std::to_string(i) + " of [B][na])"; return DOJO_ERR_INVALID; }
        }
        return DOJO_OK;
    });
}

// ... and what the constrained entries refuse (include/dojo_hip_constraints.h): the limits are optional there, the constraints record is not
static int refuse_riccati_al(DojoHandle s, int32_t H, const DojoRiccati* r, const RiccatiBox& box, const RiccatiCon* con, const char* who) {
    TRY(refuse_riccati(s, H, r, who));
    const std::string w_ = std::string(who) + ": ";
    if (!con) { g_err = w_ + "con must not be NULL"; return DOJO_ERR_INVALID; }
    if (con->nc < 0) { g_err = w_ + "nc must be >= 0"; return DOJO_ERR_INVALID; }
    if (con->nc > 0 && (!con->Cx || !con->w || !con->y)) { g_err = w_ + "Cx, w and y must not be NULL with nc > 0"; return DOJO_ERR_INVALID; }
    if (box.lim && !box.U) { g_err = w_ + "U must not be NULL with limits"; return DOJO_ERR_INVALID; }
    const int n = 2 * (int)s->M.nu, m = r->na;
    const size_t lds = dj::riccati::al_lds_bytes(n, m);
    if (lds > 65536) {
        g_err = w_ + "n = " + std::to_string(n) + ", na = " + std::to_string(m) + " needs " + std::to_string(lds) + " bytes of LDS per environment with the box QP; the kernel holds at most 65536";
        return DOJO_ERR_UNSUPPORTED;
    }
    return DOJO_OK;
}
// the weights and multipliers of a host entry are read: w < 0 and NaN are refused (the device entry cannot look)
static int refuse_constraint_values(DojoHandle s, const RiccatiCon* con, size_t count, const char* who) {
    return by_dtype(s, [&](auto t) {
        using T = decltype(t);
        const T* const w = (const T*)con->w; const T* const y = (const T*)con->y;
        for (size_t i = 0; i < count; ++i)
            if (!((double)w[i] >= 0.0) || (double)y[i] != (double)y[i]) {
                g_err = std::string(who) + ": w must be >= 0 and w, y must not be NaN (element " + std::to_string(i) + " of [H+1][B][nc])"; return DOJO_ERR_INVALID;
            }
        return DOJO_OK;
    });
}

// box = null: dojo_riccati_dev; con != null (with a box whose lim and U may be null): dojo_riccati_al_dev
static int riccati_dev(DojoHandle s, int32_t H, const DojoRiccati* r, const RiccatiBox* box, const RiccatiCon* con, bool al, void* stream, const char* who) {
    Enter enter_(s);
    TRY(al ? refuse_riccati_al(s, H, r, *box, con, who) : box ? refuse_riccati_box(s, H, r, *box, who) : refuse_riccati(s, H, r, who));
    HIPCHK(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    TRY(join_groups(s, st));                  // (asynchronous steps still in flight: the last dojo_minimal_gradients_dev may be writing the record)
    const RiccatiCon c = al ? *con : RiccatiCon{};      // (the caller's struct is read during the call only)
    return by_dtype(s, [&](auto t) { return launch_riccati_any<decltype(t)>(s, H, *r, box, al ? &c : nullptr, st); });
}
int dojo_riccati_dev(DojoHandle s, int32_t H, const DojoRiccati* r, void* stream) { return riccati_dev(s, H, r, nullptr, nullptr, false, stream, "dojo_riccati_dev"); }
int dojo_riccati_box_dev(DojoHandle s, int32_t H, const DojoRiccati* r, const DojoControlLimits* lim, const void* U, int64_t* active, int32_t* qp_iters, void* stream) {
    const RiccatiBox box{lim, U, active, qp_iters};
    return riccati_dev(s, H, r, &box, nullptr, false, stream, "dojo_riccati_box_dev");
}
int dojo_riccati_al_dev(DojoHandle s, int32_t H, const DojoRiccati* r, const DojoControlLimits* lim, const void* U, const DojoStageConstraints* con, int64_t* active, int32_t* qp_iters,
                        void* stream) {
    const RiccatiBox box{lim, U, active, qp_iters};
    return riccati_dev(s, H, r, &box, con, true, stream, "dojo_riccati_al_dev");
}

// host pointers: upload, one launch, download
static int riccati_host(DojoHandle s, int32_t H, const DojoRiccati* r, const RiccatiBox* box, const RiccatiCon* con, bool al, const char* who) {
    Enter enter_(s);
    TRY(al ? refuse_riccati_al(s, H, r, *box, con, who) : box ? refuse_riccati_box(s, H, r, *box, who) : refuse_riccati(s, H, r, who));
    HIPCHK(hipSetDevice(s->device));
    const size_t B = s->B, w = s->w, nu = s->M.nu, n = 2 * nu, m = (size_t)r->na, HB = (size_t)H * B, nc = al ? (size_t)con->nc : 0;
    if (box && box->lim) TRY(refuse_limit_values(s, box->lim, B * m, who));
    if (nc) TRY(refuse_constraint_values(s, con, (HB + B) * nc, who));
    Staging st;
    const auto &dA = st.input(HB * n * n * w, r->A), &dB = st.input(HB * n * nu * w, r->Bm), &dS = st.input(HB * sizeof(int32_t), r->status);
    const auto &dlx = st.input((HB + B) * n * w, r->lx), &dlu = st.input(HB * m * w, r->lu), &dlxx = st.input((HB + B) * n * n * w, r->lxx);
    const auto &dluu = st.input(HB * m * m * w, r->luu), &dlux = st.input(HB * m * n * w, r->lux), &dmu = st.input(B * w, r->mu);
    const auto &dlo = st.input(B * m * w, box && box->lim ? box->lim->lo : nullptr), &dhi = st.input(B * m * w, box && box->lim ? box->lim->hi : nullptr), &dU = st.input(HB * nu * w, box ? box->U : nullptr);
    const bool sh = nc && con->shared;
    const auto &dCx = st.input((sh ? 1 : HB + B) * nc * n * w, nc ? con->Cx : nullptr), &dCu = st.input((sh ? 1 : HB) * nc * m * w, nc ? con->Cu : nullptr);
    const auto &dw = st.input((HB + B) * nc * w, nc ? con->w : nullptr), &dy = st.input((HB + B) * nc * w, nc ? con->y : nullptr);
    const auto &dK = st.output(HB * m * n * w, r->K), &dk = st.output(HB * m * w, r->kff), &dF = st.output(B * sizeof(int32_t), r->fail);
    const auto &ddV = st.output(B * 2 * w, r->dV), &dVx = st.output(B * n * w, r->Vx), &dVxx = st.output(B * n * n * w, r->Vxx);
    const auto &dact = st.output(HB * sizeof(int64_t), box ? box->active : nullptr), &dit = st.output(HB * sizeof(int32_t), box ? box->qp_iters : nullptr);
    TRY(st.allocate());
    DojoRiccati d = *r;
    d.A = dA.p; d.Bm = dB.p; d.status = (const int32_t*)dS.p; d.lx = dlx.p; d.lu = dlu.p; d.lxx = dlxx.p; d.luu = dluu.p; d.lux = dlux.p; d.mu = dmu.p;
    d.K = dK.p; d.kff = dk.p; d.fail = (int32_t*)dF.p; d.dV = ddV.p; d.Vx = dVx.p; d.Vxx = dVxx.p;
    const DojoControlLimits dlim{dlo.p, dhi.p};
    const RiccatiBox dbox{box && box->lim ? &dlim : nullptr, dU.p, (int64_t*)dact.p, (int32_t*)dit.p};
    const RiccatiCon dcon{dCx.p, dCu.p, dw.p, dy.p, (int32_t)nc, al ? con->shared : 0};
    TRY(riccati_dev(s, H, &d, box ? &dbox : nullptr, al ? &dcon : nullptr, al, nullptr, who));
    return st.finish();      // (no state: the handle's own is left alone)
}
int dojo_riccati(DojoHandle s, int32_t H, const DojoRiccati* r) { return riccati_host(s, H, r, nullptr, nullptr, false, "dojo_riccati"); }
int dojo_riccati_box(DojoHandle s, int32_t H, const DojoRiccati* r, const DojoControlLimits* lim, const void* U, int64_t* active, int32_t* qp_iters) {
    const RiccatiBox box{lim, U, active, qp_iters};
    return riccati_host(s, H, r, &box, nullptr, false, "dojo_riccati_box");
}
int dojo_riccati_al(DojoHandle s, int32_t H, const DojoRiccati* r, const DojoControlLimits* lim, const void* U, const DojoStageConstraints* con, int64_t* active, int32_t* qp_iters) {
    const RiccatiBox box{lim, U, active, qp_iters};
    return riccati_host(s, H, r, &box, con, true, "dojo_riccati_al");
}

// ---- rollouts in minimal coordinates with the tracking controller (dojo_tracking.hpp, include/dojo_hip_trajopt.h): iLQR's forward pass and its linearization, one call each ----
// what both entries refuse, before anything is allocated or launched
static int refuse_tracking(DojoHandle s, int32_t H, const DojoTracking* t, const char* who) {
    const std::string w_ = std::string(who) + ": ";
    if (!s || !t) { g_err = w_ + "bad argument (the handle and the DojoTracking record are required)"; return DOJO_ERR_INVALID; }
    if (H < 1) { g_err = w_ + "H must be >= 1"; return DOJO_ERR_INVALID; }
    if (!t->x0 || !t->X || !t->U_out) { g_err = w_ + "x0, X and U_out must not be NULL"; return DOJO_ERR_INVALID; }
    if (s->M.nu == 0) { g_err = w_ + "the mechanism has no inputs"; return DOJO_ERR_INVALID; }
    if (t->na < 1 || t->act_off < 0 || (long long)t->act_off + t->na > (long long)s->M.nu) { g_err = w_ + "the controller must drive inputs act_off .. act_off + na - 1 inside 0 .. nu - 1, na >= 1"; return DOJO_ERR_INVALID; }
    if ((t->A == nullptr) != (t->Bm == nullptr)) { g_err = w_ + "A and Bm must both be given or both be NULL"; return DOJO_ERR_INVALID; }
    TRY(refuse_minimal(s, who));
    if (t->A) TRY(refuse_record(s, who));
    return DOJO_OK;      // (the controller keeps nothing in LDS: there is no shape it cannot hold)
}

// boxed: the clamped law of include/dojo_hip_limits.h, lim required
static int rollout_minimal_dev(DojoHandle s, int32_t H, const DojoTracking* t, bool boxed, const DojoControlLimits* lim, void* stream, const char* who) {
    Enter enter_(s);
    TRY(refuse_tracking(s, H, t, who));
    if (boxed && !lim) { g_err = std::string(who) + ": lim must not be NULL"; return DOJO_ERR_INVALID; }
    const DojoTracking tr = *t;      // (the caller's structs are read during the call only)
    const DojoControlLimits lm = boxed ? *lim : DojoControlLimits{nullptr, nullptr};
    Controller c; c.tracking = &tr; c.limits = boxed ? &lm : nullptr;
    RolloutIO io; io.z0 = tr.x0; io.U = tr.Ubar; io.status = tr.status; io.controller = &c; io.OBS = tr.X; io.U_out = tr.U_out; io.A = tr.A; io.Bm = tr.Bm;
    return rollout_core(s, H, io, stream);
}
int dojo_rollout_minimal_dev(DojoHandle s, int32_t H, const DojoTracking* t, void* stream) { return rollout_minimal_dev(s, H, t, false, nullptr, stream, "dojo_rollout_minimal_dev"); }
int dojo_rollout_minimal_box_dev(DojoHandle s, int32_t H, const DojoTracking* t, const DojoControlLimits* lim, void* stream) {
    return rollout_minimal_dev(s, H, t, true, lim, stream, "dojo_rollout_minimal_box_dev");
}

// host pointers (the members of *t and *lim): upload, roll out on the device, download
static int rollout_minimal_host(DojoHandle s, int32_t H, const DojoTracking* t, bool boxed, const DojoControlLimits* lim, const char* who) {
    Enter enter_(s);
    TRY(refuse_tracking(s, H, t, who));
    if (boxed && !lim) { g_err = std::string(who) + ": lim must not be NULL"; return DOJO_ERR_INVALID; }
    HIPCHK(hipSetDevice(s->device));
    const size_t B = s->B, w = s->w, nu = s->M.nu, n = 2 * nu, m = (size_t)t->na, HB = (size_t)H * B;
    if (boxed) TRY(refuse_limit_values(s, lim, B * m, who));
    Staging st;
    const auto &dx0 = st.input(B * n * w, t->x0), &dUb = st.input(HB * nu * w, t->Ubar), &dXb = st.input((HB + B) * n * w, t->Xbar);
    const auto &dK = st.input(HB * m * n * w, t->K), &dk = st.input(HB * m * w, t->kff), &da = st.input(B * w, t->alpha);
    const auto &dlo = st.input(B * m * w, boxed ? lim->lo : nullptr), &dhi = st.input(B * m * w, boxed ? lim->hi : nullptr);
    const auto &dX = st.output((HB + B) * n * w, t->X), &dU = st.output(HB * nu * w, t->U_out), &dS = st.output(HB * sizeof(int32_t), t->status);
    const auto &dA = st.output(HB * n * n * w, t->A), &dB = st.output(HB * n * nu * w, t->Bm);
    TRY(st.allocate());
    DojoTracking d = *t;
    d.x0 = dx0.p; d.Ubar = dUb.p; d.Xbar = dXb.p; d.K = dK.p; d.kff = dk.p; d.alpha = da.p;
    d.X = dX.p; d.U_out = dU.p; d.status = (int32_t*)dS.p; d.A = dA.p; d.Bm = dB.p;
    const DojoControlLimits dlim{dlo.p, dhi.p};
    TRY(rollout_minimal_dev(s, H, &d, boxed, &dlim, nullptr, who));
    return st.finish();      // (the handle keeps the last step's states itself)
}
int dojo_rollout_minimal(DojoHandle s, int32_t H, const DojoTracking* t) { return rollout_minimal_host(s, H, t, false, nullptr, "dojo_rollout_minimal"); }
int dojo_rollout_minimal_box(DojoHandle s, int32_t H, const DojoTracking* t, const DojoControlLimits* lim) { return rollout_minimal_host(s, H, t, true, lim, "dojo_rollout_minimal_box"); }

// ---- the line search side by side (include/dojo_hip_linesearch.h): T trials of P problems in one rollout, and the selection kernel (dojo_linesearch.hpp) ----
// what the fan refuses on top of refuse_tracking; *P: the problems
static int refuse_fan(DojoHandle s, int32_t H, int32_t T, const DojoTracking* t, const char* who) {
    TRY(refuse_tracking(s, H, t, who));
    const std::string w_ = std::string(who) + ": ";
    if (T < 1) { g_err = w_ + "T must be >= 1"; return DOJO_ERR_INVALID; }
    if (s->B % (size_t)T != 0) { g_err = w_ + "the batch (" + std::to_string(s->B) + ") must be T (" + std::to_string(T) + ") trials of P problems: B mod T != 0"; return DOJO_ERR_INVALID; }
    if (t->A || t->Bm) { g_err = w_ + "A and Bm must be NULL (the fan does not record Jacobians)"; return DOJO_ERR_INVALID; }
    return DOJO_OK;
}
int dojo_rollout_minimal_fan_dev(DojoHandle s, int32_t H, int32_t T, const DojoTracking* t, const DojoControlLimits* lim, void* stream) {
    Enter enter_(s);
    TRY(refuse_fan(s, H, T, t, "dojo_rollout_minimal_fan_dev"));
    const DojoTracking tr = *t;      // (the caller's structs are read during the call only)
    const DojoControlLimits lm = lim ? *lim : DojoControlLimits{nullptr, nullptr};
    Controller c; c.tracking = &tr; c.limits = lim ? &lm : nullptr; c.fan_P = (int)(s->B / (size_t)T);
    // (no io.U: rollout_core strides the feed-forward controls by B, the fan's Ubar has P rows per step -- launch_tracking takes them from the record)
    RolloutIO io; io.z0 = tr.x0; io.status = tr.status; io.controller = &c; io.OBS = tr.X; io.U_out = tr.U_out;
    return rollout_core(s, H, io, stream);
}
int dojo_rollout_minimal_fan(DojoHandle s, int32_t H, int32_t T, const DojoTracking* t, const DojoControlLimits* lim) {
    Enter enter_(s);
    const char* who = "dojo_rollout_minimal_fan";
    TRY(refuse_fan(s, H, T, t, who));
    HIPCHK(hipSetDevice(s->device));
    const size_t B = s->B, P = B / (size_t)T, w = s->w, nu = s->M.nu, n = 2 * nu, m = (size_t)t->na, HB = (size_t)H * B, HP = (size_t)H * P;
    if (lim) TRY(refuse_limit_values(s, lim, P * m, who));
    Staging st;
    const auto &dx0 = st.input(P * n * w, t->x0), &dUb = st.input(HP * nu * w, t->Ubar), &dXb = st.input((HP + P) * n * w, t->Xbar);
    const auto &dK = st.input(HP * m * n * w, t->K), &dk = st.input(HP * m * w, t->kff), &da = st.input(B * w, t->alpha);
    const auto &dlo = st.input(P * m * w, lim ? lim->lo : nullptr), &dhi = st.input(P * m * w, lim ? lim->hi : nullptr);
    const auto &dX = st.output((HB + B) * n * w, t->X), &dU = st.output(HB * nu * w, t->U_out), &dS = st.output(HB * sizeof(int32_t), t->status);
    TRY(st.allocate());
    DojoTracking d = *t;
    d.x0 = dx0.p; d.Ubar = dUb.p; d.Xbar = dXb.p; d.K = dK.p; d.kff = dk.p; d.alpha = da.p; d.X = dX.p; d.U_out = dU.p; d.status = (int32_t*)dS.p;
    const DojoControlLimits dlim{dlo.p, dhi.p};
    TRY(dojo_rollout_minimal_fan_dev(s, H, T, &d, lim ? &dlim : nullptr, nullptr));
    return st.finish();      // (the handle keeps the last step's states itself)
}

// what both selection entries refuse, before anything is allocated or launched
static int refuse_select(DojoHandle s, int32_t H, int32_t T, const DojoQuadraticCost* cost, const DojoLineSearch* ls, const char* who) {
    const std::string w_ = std::string(who) + ": ";
    if (!s || !ls) { g_err = w_ + "bad argument (the handle and the DojoLineSearch record are required)"; return DOJO_ERR_INVALID; }
    if (H < 1) { g_err = w_ + "H must be >= 1"; return DOJO_ERR_INVALID; }
    if (T < 1 || T > dj::linesearch::MAX_T) { g_err = w_ + "T must be 1 .. " + std::to_string(dj::linesearch::MAX_T) + " (the kernel keeps the trials' costs in LDS)"; return DOJO_ERR_INVALID; }
    if (s->B % (size_t)T != 0) { g_err = w_ + "the batch (" + std::to_string(s->B) + ") must be T (" + std::to_string(T) + ") trials of P problems: B mod T != 0"; return DOJO_ERR_INVALID; }
    if (!ls->X || !ls->U || !ls->alpha || !ls->dV || !ls->Xcur || !ls->Ucur || !ls->choice || !ls->alpha_acc || !ls->J_acc) {
        g_err = w_ + "X, U, alpha, dV, Xcur, Ucur, choice, alpha_acc and J_acc must not be NULL"; return DOJO_ERR_INVALID;
    }
    if (!ls->J_trial) { g_err = w_ + "J_trial must not be NULL (an output with a cost, an input without)"; return DOJO_ERR_INVALID; }
    if (!cost && !ls->J0) { g_err = w_ + "J0 must not be NULL without a cost"; return DOJO_ERR_INVALID; }
    if (cost && (!cost->Q || !cost->R || !cost->Qf || !cost->goal)) { g_err = w_ + "Q, R, Qf and goal of the cost must not be NULL"; return DOJO_ERR_INVALID; }
    if (s->M.nu == 0) { g_err = w_ + "the mechanism has no inputs"; return DOJO_ERR_INVALID; }
    if (ls->na < 1 || ls->act_off < 0 || (long long)ls->act_off + ls->na > (long long)s->M.nu) { g_err = w_ + "the cost must cover inputs act_off .. act_off + na - 1 inside 0 .. nu - 1, na >= 1"; return DOJO_ERR_INVALID; }
    if (!std::isfinite(ls->c1)) { g_err = w_ + "c1 must be finite"; return DOJO_ERR_INVALID; }
    return DOJO_OK;
}
int dojo_linesearch_select_dev(DojoHandle s, int32_t H, int32_t T, const DojoQuadraticCost* cost, const DojoLineSearch* ls, void* stream) {
    Enter enter_(s);
    TRY(refuse_select(s, H, T, cost, ls, "dojo_linesearch_select_dev"));
    HIPCHK(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    TRY(join_groups(s, st));                  // (asynchronous steps still in flight may be writing the trials)
    return by_dtype(s, [&](auto t) { return launch_select<decltype(t)>(s, H, T, cost, *ls, st); });
}
int dojo_linesearch_select(DojoHandle s, int32_t H, int32_t T, const DojoQuadraticCost* cost, const DojoLineSearch* ls) {
    Enter enter_(s);
    TRY(refuse_select(s, H, T, cost, ls, "dojo_linesearch_select"));
    HIPCHK(hipSetDevice(s->device));
    const size_t B = s->B, P = B / (size_t)T, w = s->w, nu = s->M.nu, n = 2 * nu, m = (size_t)ls->na, HB = (size_t)H * B, HP = (size_t)H * P;
    Staging st;
    const auto &dX = st.input((HB + B) * n * w, ls->X), &dU = st.input(HB * nu * w, ls->U), &dS = st.input(HB * sizeof(int32_t), ls->status);
    const auto &da = st.input(B * w, ls->alpha), &ddV = st.input(P * 2 * w, ls->dV), &dok = st.input(P * sizeof(int32_t), ls->ok);
    const auto &dXc = st.input((HP + P) * n * w, ls->Xcur), &dUc = st.input(HP * nu * w, ls->Ucur), &dJ0 = st.input(P * sizeof(double), ls->J0);
    const auto &dQ = st.input(n * n * w, cost ? cost->Q : nullptr), &dR = st.input(m * m * w, cost ? cost->R : nullptr), &dQf = st.input(n * n * w, cost ? cost->Qf : nullptr);
    const auto &dg = st.input((cost && cost->goal_per_problem ? P : 1) * n * w, cost ? cost->goal : nullptr);
    const auto &dJt = cost ? st.output(B * sizeof(double), ls->J_trial) : st.input(B * sizeof(double), ls->J_trial);
    const auto &dJc = st.output(P * sizeof(double), ls->J_cur), &dJa = st.output(P * sizeof(double), ls->J_acc);
    const auto &dch = st.output(P * sizeof(int32_t), ls->choice), &daa = st.output(P * w, ls->alpha_acc);
    const auto &dXn = st.output((HP + P) * n * w, ls->X_new), &dUn = st.output(HP * nu * w, ls->U_new);
    TRY(st.allocate());
    DojoLineSearch d = *ls;
    d.X = dX.p; d.U = dU.p; d.status = (const int32_t*)dS.p; d.alpha = da.p; d.dV = ddV.p; d.ok = (const int32_t*)dok.p; d.Xcur = dXc.p; d.Ucur = dUc.p;
    d.J0 = (const double*)dJ0.p; d.J_trial = (double*)dJt.p; d.J_cur = (double*)dJc.p; d.J_acc = (double*)dJa.p; d.choice = (int32_t*)dch.p; d.alpha_acc = daa.p;
    d.X_new = dXn.p; d.U_new = dUn.p;
    const DojoQuadraticCost dc{dQ.p, dR.p, dQf.p, dg.p, cost ? cost->goal_per_problem : 0};
    TRY(dojo_linesearch_select_dev(s, H, T, cost ? &dc : nullptr, &d, nullptr));
    return st.finish();      // (no state: the handle's own is left alone)
}

// ---- reverse mode through closed-loop rollouts (dojo_policy_adjoint.hpp) ----
int dojo_observation_jacobian_dev(DojoHandle s, const void* z, int32_t n, double* M, void* stream) {
    Enter enter_(s);
    if (!s || !z || !M || n < 1) { g_err = "dojo_observation_jacobian_dev: bad argument (handle, z and M are required, n >= 1)"; return DOJO_ERR_INVALID; }
    if (s->M.nu == 0) { g_err = "dojo_observation_jacobian_dev: the mechanism has no inputs"; return DOJO_ERR_INVALID; }
    TRY(refuse_minimal(s, "dojo_observation_jacobian_dev", ""));
    HIPCHK(hipSetDevice(s->device));
    return launch_observation_jacobian(s, z, (const char*)z + (size_t)s->B * 13 * s->M.Nb * s->w, n, M, (hipStream_t)stream);
}

int dojo_observation_jacobian(DojoHandle s, const void* z, double* M) {
    Enter enter_(s);
    if (!s || !z || !M) { g_err = "dojo_observation_jacobian: bad argument (handle, z and M are required)"; return DOJO_ERR_INVALID; }
    if (s->M.nu == 0) { g_err = "dojo_observation_jacobian: the mechanism has no inputs"; return DOJO_ERR_INVALID; }
    TRY(refuse_minimal(s, "dojo_observation_jacobian", ""));
    HIPCHK(hipSetDevice(s->device));
    const size_t zb = (size_t)s->B * 13 * s->M.Nb * s->w, mb = (size_t)s->B * 2 * s->M.nu * 24 * sizeof(double);
    Staging st;
    const auto &dz = st.input(zb, z), &dM = st.output(mb, M);
    TRY(st.allocate());
    TRY(launch_observation_jacobian(s, dz.p, nullptr, 1, (double*)dM.p, nullptr));
    return st.finish();
}

int dojo_rollout_policy_record_dev(DojoHandle s, const void* z0, const DojoPolicy* policy, int32_t H, void* Z, void* OBS, void* U_out, int32_t* status,
                                   void* DZ, void* DU, void* stream) {
    Enter enter_(s);
    TRY(refuse_policy(s, z0, policy, H, "dojo_rollout_policy_record_dev"));
    if (!Z || !OBS || !U_out || !DZ || !DU) { g_err = "dojo_rollout_policy_record_dev: Z, OBS, U_out, DZ and DU are required"; return DOJO_ERR_INVALID; }
    TRY(refuse_record(s, "dojo_rollout_policy_record_dev"));
    const DojoPolicy p = *policy;
    Controller c; c.affine = &p;
    RolloutIO io; io.z0 = z0; io.U = p.U_ff; io.Z = Z; io.status = status; io.DZ = DZ; io.DU = DU; io.controller = &c; io.OBS = OBS; io.U_out = U_out;
    return rollout_core(s, H, io, stream);
}

// everything the closed-loop sweep refuses, before anything is launched or allocated (z0 of refuse_policy: not this entry's -- the policy stands in)
static int refuse_policy_adjoint(DojoHandle s, const DojoPolicy* p, int32_t H, const char* who) {
    const std::string w_ = std::string(who) + ": ";
    TRY(refuse_policy(s, p, p, H, who));
    if (p->contact_forces) {
        g_err = w_ + "contact_forces = 1 is not supported in reverse mode (the derivative of the previous step's impulses w.r.t. the state is not part of the record)";
        return DOJO_ERR_UNSUPPORTED;
    }
    if (dj::padjoint::lds_bytes(12 * s->M.Nb, (int)s->M.nu, 2 * (int)s->M.nu, p->na) > 65536) {
        g_err = w_ + "the sweep keeps 4 nx + nu + 2 nobs + na (nobs + 1) doubles in LDS, which exceeds 64 KB for this mechanism and policy"; return DOJO_ERR_UNSUPPORTED;
    }
    return DOJO_OK;
}

// the observation Jacobians of a closed-loop sweep whose caller passes none (M = NULL): of z0 and the first H - 1 states of Z -- and of the last one where the final
// observation has a cotangent --, into the handle's buffer
static int observation_jacobians(DojoHandle s, int32_t H, const void* z0, const void* Z, bool final_state, hipStream_t st, const double** M) {
    TRY(ensure_pM(s, (size_t)H));
    TRY(launch_observation_jacobian(s, z0, Z, (long long)H + (final_state ? 1 : 0), (double*)s->d_pM, st));
    *M = (const double*)s->d_pM;
    return DOJO_OK;
}

int dojo_rollout_policy_adjoint_dev(DojoHandle s, const DojoPolicy* policy, int32_t H, const DojoPolicyAdjoint* a_, void* stream) {
    Enter enter_(s);
    const char* who = "dojo_rollout_policy_adjoint_dev";
    TRY(refuse_policy_adjoint(s, policy, H, who));
    if (!a_) { g_err = std::string(who) + ": the argument record must not be NULL"; return DOJO_ERR_INVALID; }
    const DojoPolicy p = *policy; const DojoPolicyAdjoint a = *a_;      // (the caller's structs are read during the call only)
    TRY(refuse_sweep(who, H, {{!a.DZ || !a.OBS || !a.G, "DZ, OBS and G must not be NULL"}, {!a.DU, "gU, gW, gbias and gz need DU"}}, a.cot_space, a.Z,
                     {{!a.M && (!a.z0 || !a.Z), "M = NULL needs z0 and Z (the observation Jacobians are computed from them)"}}, a.DZ, a.DU, "DZ and DU"));
    HIPCHK(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    TRY(join_groups(s, st));                  // (asynchronous steps still in flight: they may be writing the record)
    if (!a.gW && !a.gbias && !a.gU && !a.gz) return DOJO_OK;
    const double* M = a.M;
    if (!M) TRY(observation_jacobians(s, H, a.z0, a.Z, a.G_obs != nullptr, st, &M));
    double* acc = nullptr;
    if (!p.per_env) { TRY(ensure_pacc(s, (size_t)p.na)); acc = s->d_pacc; }
    return by_dtype(s, [&](auto t) { return launch_policy_adjoint<decltype(t)>(s, p, H, a, M, acc, st); });
}

// host pointers (the members of *policy too): upload, record on the device, sweep, download -- neither the Jacobians nor M cross PCIe
int dojo_rollout_policy_gradients(DojoHandle s, const void* z0, const DojoPolicy* policy, int32_t H, const void* G, int32_t cot_space, const void* G_u, const void* G_obs,
                                  void* Z, void* OBS, void* U_out, int32_t* status, void* gW, void* gbias, void* gU, void* gz) {
    Enter enter_(s);
    const char* who = "dojo_rollout_policy_gradients";
    const std::string w_ = std::string(who) + ": ";
    TRY(refuse_policy(s, z0, policy, H, who));
    TRY(refuse_policy_adjoint(s, policy, H, who));
    if (!G || (cot_space != 0 && cot_space != 1)) { g_err = w_ + "G is required and cot_space must be 0 (tangent) or 1 (state)"; return DOJO_ERR_INVALID; }
    TRY(refuse_record(s, who));
    HIPCHK(hipSetDevice(s->device));
    const size_t B = s->B, w = s->w, nz = 13 * s->M.Nb, nx = 12 * s->M.Nb, nu = s->M.nu, HB = (size_t)H * B, ng = cot_space ? nz : nx;
    const size_t na = (size_t)policy->na, Bw = policy->per_env ? B : 1, nobs = 2 * nu;
    Staging st;
    const auto &dz0 = st.input(B * nz * w, z0), &dW = st.input(Bw * na * nobs * w, policy->W), &db = st.input(Bw * na * w, policy->bias);
    const auto &dm = st.input(nobs * w, policy->mean), &dsc = st.input(nobs * w, policy->scale), &dUff = st.input(HB * nu * w, policy->U_ff);
    const auto &dG = st.input(HB * ng * w, G), &dGu = st.input(HB * nu * w, G_u), &dGo = st.input((HB + B) * nobs * w, G_obs);
    const auto &dZ = st.kept(HB * nz * w, Z), &dO = st.kept((HB + B) * nobs * w, OBS), &dU = st.kept(HB * nu * w, U_out), &dS = st.kept(HB * sizeof(int), status);
    const auto &dDZ = st.kept(HB * nx * nx * w), &dDU = st.kept(HB * nx * nu * w);
    const auto &dgW = st.kept(Bw * na * nobs * w, gW), &dgb = st.kept(Bw * na * w, gbias), &dgU = st.kept(HB * nu * w, gU), &dgz = st.kept(B * nx * w, gz);
    {
        Measuring handle(s);
        TRY(ensure_record(s)); TRY(ensure_pM(s, (size_t)H));
        if (!policy->per_env) TRY(ensure_pacc(s, na));
        TRY(refuse_memory(w_ + "the record of " + std::to_string(HB * nx * (nx + nu) * w) + " bytes and the observation Jacobians of " + std::to_string(pM_size(s, (size_t)H)) + " bytes (", st, handle, "do"));
    }
    TRY(st.allocate());
    DojoPolicy p = *policy; p.W = dW.p; p.bias = db.p; p.mean = dm.p; p.scale = dsc.p; p.U_ff = dUff.p;
    Controller c; c.affine = &p;
    RolloutIO io; io.z0 = dz0.p; io.U = p.U_ff; io.Z = dZ.p; io.status = (int32_t*)dS.p; io.DZ = dDZ.p; io.DU = dDU.p; io.controller = &c; io.OBS = dO.p; io.U_out = dU.p;
    TRY(rollout_core(s, H, io, nullptr));
    DojoPolicyAdjoint a{};
    a.G = dG.p; a.G_u = dGu.p; a.G_obs = dGo.p; a.DZ = dDZ.p; a.DU = dDU.p; a.OBS = dO.p; a.status = (const int32_t*)dS.p; a.z0 = dz0.p; a.Z = dZ.p; a.M = nullptr; a.cot_space = cot_space;
    a.gW = dgW.p; a.gbias = dgb.p; a.gU = dgU.p; a.gz = dgz.p;
    TRY(dojo_rollout_policy_adjoint_dev(s, &p, H, &a, nullptr));
    return st.finish(s, dZ, H);
}

// ---- closed-loop rollouts with a network policy, forward and reverse mode (dojo_mlp.hpp) ----
// Everything the forward entries refuse, before anything is launched or allocated; *sh: what the widths determine
static int refuse_mlp(DojoHandle s, const void* z0, const DojoMlpPolicy* p, int32_t H, const char* who, dj::mlp::Shape* sh) {
    const std::string w_ = std::string(who) + ": ";
    if (!s || !z0 || !p || !p->theta) { g_err = w_ + "bad argument (handle, z0, policy and policy->theta are required)"; return DOJO_ERR_INVALID; }
    const int L = p->n_layers;
    if (L < 1 || L > DOJO_MLP_MAX_LAYERS) { g_err = w_ + "n_layers must be 1 .. " + std::to_string(DOJO_MLP_MAX_LAYERS); return DOJO_ERR_INVALID; }
    for (int l = 0; l <= L; ++l)
        if (p->width[l] < 1) { g_err = w_ + "width[" + std::to_string(l) + "] must be >= 1"; return DOJO_ERR_INVALID; }
    // the affine policy with the same observation and the same driven inputs: what dojo_rollout_policy_dev refuses
    const DojoPolicy q{p->theta, nullptr, p->mean, p->scale, p->U_ff, p->per_env, p->act_off, p->width[L], p->contact_forces, p->contact_init, 0};
    TRY(refuse_policy(s, z0, &q, H, who));
    const long long nobs = 2 * (long long)s->M.nu + (p->contact_forces ? (long long)s->M.Nc : 0);
    if (p->width[0] != nobs) { g_err = w_ + "width[0] must be the number of observations, " + std::to_string(nobs); return DOJO_ERR_INVALID; }
    *sh = dj::mlp::shape(L, p->width);
    if (sh->P > 0x7fffffffLL) { g_err = w_ + "supports fewer than 2^31 parameters per policy"; return DOJO_ERR_UNSUPPORTED; }
    if (dj::mlp::lds_bytes((int)nobs, sh->nh) > 65536) {
        g_err = w_ + "the controller keeps 4 (nobs + nh) doubles in LDS (nh: the hidden units), which exceeds 64 KB for this policy"; return DOJO_ERR_UNSUPPORTED;
    }
    return DOJO_OK;
}

int dojo_rollout_mlp_dev(DojoHandle s, const void* z0, const DojoMlpPolicy* policy, int32_t H, void* Z, void* OBS, void* U_out, double* ACT, int32_t* status, void* stream) {
    Enter enter_(s);
    Controller c;
    TRY(refuse_mlp(s, z0, policy, H, "dojo_rollout_mlp_dev", &c.shape));
    const DojoMlpPolicy p = *policy;      // (the caller's struct is read during the call only)
    c.mlp = &p; c.ACT = c.shape.nh ? ACT : nullptr;
    RolloutIO io; io.z0 = z0; io.U = p.U_ff; io.Z = Z; io.status = status; io.controller = &c; io.OBS = OBS; io.U_out = U_out;
    return rollout_core(s, H, io, stream);
}

// host pointers (the members of *policy too): upload, roll out on the device, download
int dojo_rollout_mlp(DojoHandle s, const void* z0, const DojoMlpPolicy* policy, int32_t H, void* Z, void* OBS, void* U_out, int32_t* status) {
    Enter enter_(s);
    Controller c;
    TRY(refuse_mlp(s, z0, policy, H, "dojo_rollout_mlp", &c.shape));
    HIPCHK(hipSetDevice(s->device));
    const size_t B = s->B, w = s->w, nz = 13 * s->M.Nb, nu = s->M.nu, HB = (size_t)H * B, Bw = policy->per_env ? B : 1, P = (size_t)c.shape.P;
    const size_t nobs = 2 * nu + (policy->contact_forces ? (size_t)s->M.Nc : 0);
    Staging st;
    const auto &dz0 = st.input(B * nz * w, z0), &dth = st.input(Bw * P * w, policy->theta);
    const auto &dm = st.input(nobs * w, policy->mean), &dsc = st.input(nobs * w, policy->scale), &dUff = st.input(HB * nu * w, policy->U_ff);
    const auto &dZ = st.output(HB * nz * w, Z), &dO = st.output((HB + B) * nobs * w, OBS), &dU = st.output(HB * nu * w, U_out), &dS = st.output(HB * sizeof(int), status);
    TRY(st.allocate());
    DojoMlpPolicy p = *policy; p.theta = dth.p; p.mean = dm.p; p.scale = dsc.p; p.U_ff = dUff.p;
    c.mlp = &p;
    RolloutIO io; io.z0 = dz0.p; io.U = p.U_ff; io.Z = dZ.p; io.status = (int32_t*)dS.p; io.controller = &c; io.OBS = dO.p; io.U_out = dU.p;
    TRY(rollout_core(s, H, io, nullptr));
    return st.finish(s, dZ, H);
}

int dojo_rollout_mlp_record_dev(DojoHandle s, const void* z0, const DojoMlpPolicy* policy, int32_t H, void* Z, void* OBS, void* U_out, double* ACT, int32_t* status,
                                void* DZ, void* DU, void* stream) {
    Enter enter_(s);
    const char* who = "dojo_rollout_mlp_record_dev";
    Controller c;
    TRY(refuse_mlp(s, z0, policy, H, who, &c.shape));
    if (!Z || !OBS || !U_out || !DZ || !DU) { g_err = std::string(who) + ": Z, OBS, U_out, DZ and DU are required"; return DOJO_ERR_INVALID; }
    if (policy->n_layers > 1 && !ACT) { g_err = std::string(who) + ": ACT is required with n_layers > 1 (the sweep reads the activations from it)"; return DOJO_ERR_INVALID; }
    TRY(refuse_record(s, who));
    const DojoMlpPolicy p = *policy;
    c.mlp = &p; c.ACT = c.shape.nh ? ACT : nullptr;
    RolloutIO io; io.z0 = z0; io.U = p.U_ff; io.Z = Z; io.status = status; io.DZ = DZ; io.DU = DU; io.controller = &c; io.OBS = OBS; io.U_out = U_out;
    return rollout_core(s, H, io, stream);
}

// everything the network sweep refuses, before anything is launched or allocated (z0 of refuse_mlp: not this entry's -- the policy stands in)
static int refuse_mlp_adjoint(DojoHandle s, const DojoMlpPolicy* p, int32_t H, const char* who, dj::mlp::Shape* sh) {
    const std::string w_ = std::string(who) + ": ";
    TRY(refuse_mlp(s, p, p, H, who, sh));
    if (p->contact_forces) {
        g_err = w_ + "contact_forces = 1 is not supported in reverse mode (the derivative of the previous step's impulses w.r.t. the state is not part of the record)";
        return DOJO_ERR_UNSUPPORTED;
    }
    if (dj::mlp::adjoint_lds_bytes(12 * s->M.Nb, (int)s->M.nu, 2 * (int)s->M.nu, sh->wmax, sh->nh) > 65536) {
        g_err = w_ + "the sweep keeps 4 nx + nu + 2 nobs + 2 wmax + nh doubles in LDS, which exceeds 64 KB for this mechanism and policy"; return DOJO_ERR_UNSUPPORTED;
    }
    return DOJO_OK;
}

int dojo_rollout_mlp_adjoint_dev(DojoHandle s, const DojoMlpPolicy* policy, int32_t H, const DojoMlpAdjoint* a_, void* stream) {
    Enter enter_(s);
    const char* who = "dojo_rollout_mlp_adjoint_dev";
    dj::mlp::Shape sh{};
    TRY(refuse_mlp_adjoint(s, policy, H, who, &sh));
    if (!a_) { g_err = std::string(who) + ": the argument record must not be NULL"; return DOJO_ERR_INVALID; }
    const DojoMlpPolicy p = *policy; const DojoMlpAdjoint a = *a_;      // (the caller's structs are read during the call only)
    TRY(refuse_sweep(who, H, {{!a.DZ || !a.OBS || !a.G, "DZ, OBS and G must not be NULL"}, {!a.DU, "gU, gtheta and gz need DU"},
                              {p.n_layers > 1 && !a.ACT, "ACT is required with n_layers > 1 (the recorded activations)"}}, a.cot_space, a.Z,
                     {{!a.M && (!a.z0 || !a.Z), "M = NULL needs z0 and Z (the observation Jacobians are computed from them)"}}, a.DZ, a.DU, "DZ and DU"));
    HIPCHK(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    TRY(join_groups(s, st));                  // (asynchronous steps still in flight: they may be writing the record)
    if (!a.gtheta && !a.gU && !a.gz) return DOJO_OK;
    const double* M = a.M;
    if (!M) TRY(observation_jacobians(s, H, a.z0, a.Z, a.G_obs != nullptr, st, &M));
    TRY(ensure_macc(s, (size_t)sh.P));
    return by_dtype(s, [&](auto t) { return launch_mlp_adjoint<decltype(t)>(s, p, sh, H, a, M, s->d_macc, st); });
}

// host pointers (the members of *policy too): upload, record on the device, sweep, download -- the Jacobians, M and ACT do not cross PCIe
int dojo_rollout_mlp_gradients(DojoHandle s, const void* z0, const DojoMlpPolicy* policy, int32_t H, const void* G, int32_t cot_space, const void* G_u, const void* G_obs,
                               void* Z, void* OBS, void* U_out, int32_t* status, void* gtheta, void* gU, void* gz) {
    Enter enter_(s);
    const char* who = "dojo_rollout_mlp_gradients";
    const std::string w_ = std::string(who) + ": ";
    Controller c;
    if (!z0) { g_err = w_ + "bad argument (handle, z0, policy and policy->theta are required)"; return DOJO_ERR_INVALID; }
    TRY(refuse_mlp_adjoint(s, policy, H, who, &c.shape));
    if (!G || (cot_space != 0 && cot_space != 1)) { g_err = w_ + "G is required and cot_space must be 0 (tangent) or 1 (state)"; return DOJO_ERR_INVALID; }
    TRY(refuse_record(s, who));
    HIPCHK(hipSetDevice(s->device));
    const size_t B = s->B, w = s->w, nz = 13 * s->M.Nb, nx = 12 * s->M.Nb, nu = s->M.nu, HB = (size_t)H * B, ng = cot_space ? nz : nx;
    const size_t Bw = policy->per_env ? B : 1, nobs = 2 * nu, P = (size_t)c.shape.P, abytes = HB * (size_t)c.shape.nh * sizeof(double);
    Staging st;
    const auto &dz0 = st.input(B * nz * w, z0), &dth = st.input(Bw * P * w, policy->theta);
    const auto &dm = st.input(nobs * w, policy->mean), &dsc = st.input(nobs * w, policy->scale), &dUff = st.input(HB * nu * w, policy->U_ff);
    const auto &dG = st.input(HB * ng * w, G), &dGu = st.input(HB * nu * w, G_u), &dGo = st.input((HB + B) * nobs * w, G_obs);
    const auto &dZ = st.kept(HB * nz * w, Z), &dO = st.kept((HB + B) * nobs * w, OBS), &dU = st.kept(HB * nu * w, U_out), &dS = st.kept(HB * sizeof(int), status);
    const auto &dA = st.kept(abytes, nullptr, abytes != 0);      // (a single layer has no activations)
    const auto &dDZ = st.kept(HB * nx * nx * w), &dDU = st.kept(HB * nx * nu * w);
    const auto &dgth = st.kept(Bw * P * w, gtheta), &dgU = st.kept(HB * nu * w, gU), &dgz = st.kept(B * nx * w, gz);
    {
        Measuring handle(s);
        TRY(ensure_record(s)); TRY(ensure_pM(s, (size_t)H)); TRY(ensure_macc(s, P));
        TRY(refuse_memory(w_ + "the record of " + std::to_string(HB * nx * (nx + nu) * w) + " bytes, the observation Jacobians of " + std::to_string(pM_size(s, (size_t)H)) + " bytes, the activations of "
                          + std::to_string(abytes) + " bytes and the accumulators of " + std::to_string(macc_size(s, P)) + " bytes (", st, handle, "do"));
    }
    TRY(st.allocate());
    DojoMlpPolicy p = *policy; p.theta = dth.p; p.mean = dm.p; p.scale = dsc.p; p.U_ff = dUff.p;
    c.mlp = &p; c.ACT = (double*)dA.p;
    RolloutIO io; io.z0 = dz0.p; io.U = p.U_ff; io.Z = dZ.p; io.status = (int32_t*)dS.p; io.DZ = dDZ.p; io.DU = dDU.p; io.controller = &c; io.OBS = dO.p; io.U_out = dU.p;
    TRY(rollout_core(s, H, io, nullptr));
    DojoMlpAdjoint a{};
    a.G = dG.p; a.G_u = dGu.p; a.G_obs = dGo.p; a.DZ = dDZ.p; a.DU = dDU.p; a.OBS = dO.p; a.ACT = c.ACT; a.status = (const int32_t*)dS.p; a.z0 = dz0.p; a.Z = dZ.p; a.M = nullptr; a.cot_space = cot_space;
    a.gtheta = dgth.p; a.gU = dgU.p; a.gz = dgz.p;
    TRY(dojo_rollout_mlp_adjoint_dev(s, &p, H, &a, nullptr));
    return st.finish(s, dZ, H);
}

static int rollout_host(DojoHandle s, const void* z0, const void* U, int32_t H, void* Z, void* storage, int32_t* status) {
    if (!s || !z0 || H < 1) { g_err = "dojo_rollout: bad argument"; return DOJO_ERR_INVALID; }
    HIPCHK(hipSetDevice(s->device));
    const size_t B = s->B, w = s->w, nz = 13 * s->M.Nb, nu = s->M.nu, HB = (size_t)H * B;
    Staging st;
    const auto &dSt = st.output(HB * 25 * s->M.Nb * w, storage), &dz0 = st.input(B * nz * w, z0), &dU = st.input(HB * nu * w, nu ? U : nullptr);
    const auto &dZ = st.output(HB * nz * w, Z), &dS = st.output(HB * sizeof(int), status);
    TRY(st.allocate());
    RolloutIO io; io.z0 = dz0.p; io.U = dU.p; io.Z = dZ.p; io.status = (int32_t*)dS.p; io.storage = dSt.p;
    TRY(rollout_core(s, H, io, nullptr));
    return st.finish(s, dZ, H);
}

int dojo_rollout(DojoHandle s, const void* z0, const void* U, int32_t H, void* Z, int32_t* status) {
    Enter enter_(s);
    return rollout_host(s, z0, U, H, Z, nullptr, status);
}

int dojo_simulate(DojoHandle s, const void* z0, const void* U, int32_t H, void* Z, void* storage, int32_t* status) {
    Enter enter_(s);
    if (!storage) { g_err = "dojo_simulate: storage must not be NULL (use dojo_rollout for record = false)"; return DOJO_ERR_INVALID; }
    return rollout_host(s, z0, U, H, Z, storage, status);
}

int dojo_get_state(DojoHandle s, void* z) {
    Enter enter_(s);
    if (!s || !z || !s->d_zn) { g_err = "dojo_get_state: no state"; return DOJO_ERR_INVALID; }
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(z, s->d_zn, (size_t)s->B * 13 * s->M.Nb * s->w, hipMemcpyDeviceToHost));
    return DOJO_OK;
}

// ---- contact-data gradients: get_contact_gradients, src/gradients/contact.jl:1-55 ----
int dojo_contact_gradients_dev(DojoHandle s, const void* z, const void* u, void* dc, void* stream) {
    Enter enter_(s);
    if (!s || !z || !dc) { g_err = "dojo_contact_gradients_dev: bad argument"; return DOJO_ERR_INVALID; }
    if (!s->d_sol) { g_err = "dojo_contact_gradients_dev: no differentiable step (dz/du requested) has been run on this handle"; return DOJO_ERR_INVALID; }
    if (s->M.Nc == 0) return DOJO_OK;
    HIPCHK(hipSetDevice(s->device));
    int slot = -1;
    TRY(refuse_unsupported(s, false, true));
    TRY(join_groups(s, (hipStream_t)stream));
    const StepIO io{z, u, s->d_zn ? s->d_zn : (void*)z, nullptr, nullptr, nullptr, nullptr, dc, nullptr};
    return launch_any(s, io, whole_batch(s, (hipStream_t)stream), step_mode(s, 1).with(PH_ALL, &slot));
}
int dojo_contact_gradients(DojoHandle s, void* dc) {
    Enter enter_(s);
    if (!s || !dc) { g_err = "dojo_contact_gradients: bad argument"; return DOJO_ERR_INVALID; }
    if (!s->have_grad || !s->d_z) { g_err = "dojo_contact_gradients: call dojo_step(..., with_gradient = 1) first"; return DOJO_ERR_INVALID; }
    HIPCHK(hipSetDevice(s->device));
    const size_t nx = 12 * s->M.Nb, ncc = 5 * (size_t)s->M.Nc;
    if (ncc == 0) return DOJO_OK;
    Staging st;
    const auto& d_dc = st.kept((size_t)s->B * nx * ncc * s->w);
    TRY(st.allocate());
    TRY(dojo_contact_gradients_dev(s, s->d_z, s->have_u ? s->d_u : nullptr, d_dc.p, nullptr));
    TRY(st.finish());
    return download_transposed(s, dc, d_dc.p, nx, ncc);      // device layout [B][5Nc columns][12Nb rows] -> host layout [B, 12Nb, 5Nc]
}

// set_data!(mechanism.contacts, theta) (examples/system_identification/utilities.jl:52) on a live handle: theta [Nc][5] =
// [friction_coefficient, contact_radius, contact_origin(3)] per contact.  The contact table is the only place these values live (the cut element of a
// body-body contact holds the contact's index, make_globals reads none of them), so the handle then steps as one created with theta.
int dojo_set_contact_data(DojoHandle s, const double* theta) {
    Enter enter_(s);
    if (!s) { g_err = "dojo_set_contact_data: bad argument"; return DOJO_ERR_INVALID; }
    const int Nc = s->M.Nc;
    if (Nc == 0) return DOJO_OK;
    if (!theta) { g_err = "dojo_set_contact_data: theta must not be NULL"; return DOJO_ERR_INVALID; }
    for (int c = 0; c < Nc; ++c) {
        const double* t = theta + 5 * (size_t)c;
        for (int i = 0; i < 5; ++i) if (!std::isfinite(t[i])) { g_err = "dojo_set_contact_data: contact " + std::to_string(c) + " has a non-finite value"; return DOJO_ERR_INVALID; }
        if (t[0] < 0.0 || t[1] < 0.0) { g_err = "dojo_set_contact_data: contact " + std::to_string(c) + " has a negative friction coefficient or radius"; return DOJO_ERR_INVALID; }
        if (s->M.contact_model == 1 && t[0] != 0.0) {
            g_err = "dojo_set_contact_data: an ImpactContact has no friction coefficient (contact " + std::to_string(c) + ": pass 0)"; return DOJO_ERR_UNSUPPORTED;
        }
    }
    HIPCHK(hipSetDevice(s->device));
    TRY(join_groups(s, nullptr));
    HIPCHK(hipDeviceSynchronize());                          // steps still in flight read the previous table
    for (int c = 0; c < Nc; ++c) {
        dj::ContactP<double>& Q = s->M.contacts[c]; const double* t = theta + 5 * (size_t)c;
        Q.mu = t[0]; Q.r = t[1]; for (int i = 0; i < 3; ++i) Q.o[i] = t[2 + i];
    }
    std::vector<dj::ContactP<double>> contacts; for (auto& c : s->M.contacts) contacts.push_back(dj::cast_contact<double>(c));     // the contacts part of upload_tables
    HIPCHK(hipMemcpy(s->d_contacts, contacts.data(), contacts.size() * sizeof(dj::ContactP<double>), hipMemcpyHostToDevice));
    s->have_grad = false;                                    // the hand-off record holds a solution obtained with the old theta
    return DOJO_OK;
}
int dojo_get_contact_data(DojoHandle s, double* theta) {
    Enter enter_(s);
    if (!s) { g_err = "dojo_get_contact_data: bad argument"; return DOJO_ERR_INVALID; }
    if (s->M.Nc == 0) return DOJO_OK;
    if (!theta) { g_err = "dojo_get_contact_data: theta must not be NULL"; return DOJO_ERR_INVALID; }
    for (int c = 0; c < s->M.Nc; ++c) {
        const dj::ContactP<double>& Q = s->M.contacts[c]; double* t = theta + 5 * (size_t)c;
        t[0] = Q.mu; t[1] = Q.r; for (int i = 0; i < 3; ++i) t[2 + i] = Q.o[i];
    }
    return DOJO_OK;
}

// ---- minimal <-> maximal coordinates ----
int dojo_minimal_to_maximal_dev(DojoHandle s, const void* x, void* z, void* stream) {
    Enter enter_(s);
    if (!s || !x || !z) { g_err = "dojo_minimal_to_maximal_dev: bad argument"; return DOJO_ERR_INVALID; }
    TRY(refuse_minimal(s, "dojo_minimal_to_maximal_dev"));
    HIPCHK(hipSetDevice(s->device));
    TRY(join_groups(s, (hipStream_t)stream));      // (asynchronous steps still in flight may write / read these buffers)
    return by_dtype(s, [&](auto t) { return launch_min2max<decltype(t)>(s, x, z, (hipStream_t)stream); });
}
int dojo_maximal_to_minimal_dev(DojoHandle s, const void* z, void* x, void* stream) {
    Enter enter_(s);
    if (!s || !x || !z) { g_err = "dojo_maximal_to_minimal_dev: bad argument"; return DOJO_ERR_INVALID; }
    TRY(refuse_minimal(s, "dojo_maximal_to_minimal_dev"));
    HIPCHK(hipSetDevice(s->device));
    TRY(join_groups(s, (hipStream_t)stream));      // (asynchronous steps still in flight may write / read these buffers)
    return by_dtype(s, [&](auto t) { return launch_max2min<decltype(t)>(s, z, x, 2 * (int)s->M.nu, (hipStream_t)stream); });
}
// get_state(environment) of DojoEnvironments: the minimal state of z (environments.jl:100-102, quadruped_sampling.jl:67-72)
// and, with contact_forces != 0, the clamped normal impulses of the last step behind it (ant_ars.jl:72-80).
// obs [B, 2nu (+ Nc)]
int dojo_observe_dev(DojoHandle s, const void* z, void* obs, int32_t contact_forces, void* stream) {
    Enter enter_(s);
    if (!s || !obs) { g_err = "dojo_observe_dev: bad argument"; return DOJO_ERR_INVALID; }
    TRY(refuse_minimal(s, "dojo_observe_dev"));
    if (!z) z = s->d_zn;                   // the state the last host-buffer / minimal-coordinate step left on the handle
    if (!z) { g_err = "dojo_observe_dev: z is NULL and the handle holds no state yet"; return DOJO_ERR_INVALID; }
    if (contact_forces && !s->have_solution) { g_err = "dojo_observe_dev: contact forces need a step on this handle"; return DOJO_ERR_INVALID; }
    if (contact_forces && s->M.contact_model == 2) { g_err = "dojo_observe: contact forces are not available for LinearContact mechanisms"; return DOJO_ERR_UNSUPPORTED; }
    HIPCHK(hipSetDevice(s->device));
    TRY(join_groups(s, (hipStream_t)stream));
    const int Nc = contact_forces ? s->M.Nc : 0, ld = 2 * (int)s->M.nu + Nc;
    return by_dtype(s, [&](auto t) {
        using TIO = decltype(t);
        TRY(launch_max2min<TIO>(s, z, obs, ld, (hipStream_t)stream));
        return Nc ? launch_contact_obs<TIO>(s, obs, ld, (hipStream_t)stream) : DOJO_OK;
    });
}
int dojo_observe(DojoHandle s, void* obs, int32_t contact_forces) {
    Enter enter_(s);
    if (!s || !obs || !s->d_zn || !s->have_solution) { g_err = "dojo_observe: no step has been taken on this handle"; return DOJO_ERR_INVALID; }
    HIPCHK(hipSetDevice(s->device));
    const size_t ld = 2 * s->M.nu + (contact_forces ? s->M.Nc : 0), bytes = (size_t)s->B * ld * s->w;
    Staging st;
    const auto& d = st.output(bytes, obs);
    TRY(st.allocate());
    HIPCHK(hipDeviceSynchronize());                          // (not the cached stream of the last step: the caller may have destroyed it)
    TRY(dojo_observe_dev(s, s->d_zn, d.p, contact_forces, nullptr));
    return st.finish();
}
// step_minimal_coordinates!  src/simulation/step.jl:42-60: x -> z -> step! -> z' -> x'
int dojo_step_minimal_dev(DojoHandle s, const void* x, const void* u, void* x_next, int32_t* status, int32_t* iters, void* stream) {
    Enter enter_(s);
    if (!s || !x || !x_next) { g_err = "dojo_step_minimal_dev: bad argument"; return DOJO_ERR_INVALID; }
    TRY(refuse_minimal(s, "dojo_step_minimal_dev"));
    HIPCHK(hipSetDevice(s->device));
    size_t B = s->B, w = s->w, nz = 13 * s->M.Nb;
    ENSURE(s->d_z, B * nz * w); ENSURE(s->d_zn, B * nz * w);
    // (asynchronous handle: environment groups of the previous call may still read d_z / write d_zn, and the kernels that follow
    //  the step on `stream` read what its groups write -- both sides of the step are joined into the caller's stream here)
    TRY(join_groups(s, (hipStream_t)stream));
    TRY(dojo_minimal_to_maximal_dev(s, x, s->d_z, stream));
    TRY(dojo_step_dev(s, s->d_z, u, s->d_zn, status, iters, nullptr, nullptr, stream));
    TRY(join_groups(s, (hipStream_t)stream));
    s->have_grad = false;
    return dojo_maximal_to_minimal_dev(s, s->d_zn, x_next, stream);
}
// get_minimal_gradients!(mechanism, y, u; opts)  src/gradients/state.jl:183-217: steps in minimal coordinates and chains
//   max_to_min_jacobian(z+) * maximal Jacobians * min_to_max_jacobian(x).
// DOJO_GRAD_REFERENCE reproduces the reference literally: after its update_state! the "current" state is already the new
// one, so it evaluates min_to_max at maximal_to_minimal(z_new) and max_to_min at get_next_state = z_new advanced by one
// more integrator step.  DOJO_GRAD_CONSISTENT: min_to_max at x, max_to_min at z_new.
// jx [B][2nu][2nu], ju [B][2nu][nu] row-major per environment.
int dojo_minimal_gradients_dev(DojoHandle s, const void* x, const void* u, void* x_next, int32_t* status, int32_t* iters,
                               void* jx, void* ju, void* stream) {
    Enter enter_(s);
    if (!s || !x || !x_next || !jx) { g_err = "dojo_minimal_gradients_dev: bad argument"; return DOJO_ERR_INVALID; }
    TRY(refuse_minimal(s, "dojo_minimal_gradients_dev"));
    HIPCHK(hipSetDevice(s->device));
    const size_t B = s->B, w = s->w, Nb = s->M.Nb, nz = 13 * Nb, nx = 12 * Nb, nu = s->M.nu, nm = 2 * nu;
    hipStream_t st = (hipStream_t)stream;
    ENSURE(s->d_z, B * nz * w); ENSURE(s->d_zn, B * nz * w);
    ENSURE(s->d_dz, B * nx * nx * w); ENSURE(s->d_du, B * nx * (nu + 1) * w);
    ENSURE(s->d_jm, B * nx * (nm + 1) * sizeof(double)); ENSURE(s->d_jt, B * nx * (nm + 1) * sizeof(double));
    ENSURE(s->d_jb, B * Nb * 12 * 24 * sizeof(double));
    TRY(join_groups(s, st));              // (asynchronous handle: see dojo_step_minimal_dev)
    TRY(dojo_minimal_to_maximal_dev(s, x, s->d_z, stream));
    TRY(dojo_step_dev(s, s->d_z, u, s->d_zn, status, iters, s->d_dz, s->d_du, stream));
    TRY(join_groups(s, st));
    s->have_grad = false;          // the hand-off belongs to (d_z, the CALLER's u): the host variant below re-arms the flag with its own copy of u
    TRY(dojo_maximal_to_minimal_dev(s, s->d_zn, x_next, stream));
    const bool literal = s->grad_mode == DOJO_GRAD_REFERENCE;
    const void* xj = literal ? (const void*)x_next : x;                // where the min -> max Jacobian is evaluated ...
    const void* zj = literal ? (const void*)s->d_zn : (const void*)s->d_z;   // ... and the maximal state that belongs to it
    return by_dtype(s, [&](auto t) { return launch_minimal_chain<decltype(t)>(s, whole_batch(s, st), xj, zj, literal ? 1 : 0, jx, ju); });
}
int dojo_minimal_gradients(DojoHandle s, const void* x, const void* u, void* x_next, int32_t* status, int32_t* iters, void* jx, void* ju) {
    Enter enter_(s);
    if (!s || !x || !x_next || !jx) { g_err = "dojo_minimal_gradients: bad argument"; return DOJO_ERR_INVALID; }
    HIPCHK(hipSetDevice(s->device));
    const size_t B = s->B, w = s->w, nu = s->M.nu, nm = 2 * nu;
    const void* d_u = nullptr;
    ENSURE(s->d_x, B * (nm + 1) * w); ENSURE(s->d_xn, B * (nm + 1) * w);
    Staging st;
    const auto &d_jx = st.output(B * nm * nm * w, jx), &d_ju = st.kept(B * nm * nu * w, nu ? ju : nullptr);
    TRY(st.allocate());
    TRY(upload_step(s, s->d_x, x, nm, u, &d_u));
    TRY(dojo_minimal_gradients_dev(s, s->d_x, d_u, s->d_xn, s->d_status, s->d_iters, d_jx.p, d_ju.p, nullptr));
    s->have_grad = true; s->have_u = (u && nu);   // d_z, d_u, d_dz, d_du and the hand-off all belong to this step
    TRY(download_step(s, x_next, s->d_xn, nm, status, iters));
    return st.finish();
}

static int coords_host(DojoHandle s, const void* in, void* out, size_t n_in, size_t n_out, bool to_max) {
    HIPCHK(hipSetDevice(s->device));
    size_t B = s->B, w = s->w;
    ENSURE(s->d_x, B * (2 * s->M.nu + 1) * w);
    ENSURE(s->d_cz, B * 13 * s->M.Nb * w);       // not d_z: that is the state dojo_contact_gradients re-linearizes at
    void* din = to_max ? s->d_x : s->d_cz; void* dout = to_max ? s->d_cz : s->d_x;
    HIPCHK(hipMemcpy(din, in, B * n_in * w, hipMemcpyHostToDevice));
    TRY(to_max ? dojo_minimal_to_maximal_dev(s, din, dout, nullptr) : dojo_maximal_to_minimal_dev(s, din, dout, nullptr));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, dout, B * n_out * w, hipMemcpyDeviceToHost));
    return DOJO_OK;
}
int dojo_minimal_to_maximal(DojoHandle s, const void* x, void* z) {
    Enter enter_(s);
    if (!s || !x || !z) { g_err = "dojo_minimal_to_maximal: bad argument"; return DOJO_ERR_INVALID; }
    return coords_host(s, x, z, 2 * s->M.nu, 13 * s->M.Nb, true);
}
int dojo_maximal_to_minimal(DojoHandle s, const void* z, void* x) {
    Enter enter_(s);
    if (!s || !x || !z) { g_err = "dojo_maximal_to_minimal: bad argument"; return DOJO_ERR_INVALID; }
    return coords_host(s, z, x, 13 * s->M.Nb, 2 * s->M.nu, false);
}
// The vector the reference's step! literally RETURNS (src/simulation/step.jl:28: get_next_state after update_state!, SURVEY.md
// §8a Q1): the internal state z_next = (x3, v25, q3, ω25) advanced once more with its own velocities, (x3 + Δt v25, v25,
// q3 ⊗ ξ(ω25), ω25).  dojo_step returns the internal state; a caller that wants the literal return applies this to it.
int dojo_next_state_dev(DojoHandle s, const void* z, void* z_out, void* stream) {
    Enter enter_(s);
    if (!s || !z || !z_out) { g_err = "dojo_next_state_dev: bad argument"; return DOJO_ERR_INVALID; }
    HIPCHK(hipSetDevice(s->device));
    TRY(join_groups(s, (hipStream_t)stream));      // (asynchronous steps still in flight may write / read these buffers)
    return by_dtype(s, [&](auto t) { return launch_next_state<decltype(t)>(s, z, z_out, (hipStream_t)stream); });
}
int dojo_next_state(DojoHandle s, const void* z, void* z_out) {
    Enter enter_(s);
    if (!s || !z || !z_out) { g_err = "dojo_next_state: bad argument"; return DOJO_ERR_INVALID; }
    HIPCHK(hipSetDevice(s->device));
    const size_t bytes = (size_t)s->B * 13 * s->M.Nb * s->w;
    Staging st;
    const auto &a = st.input(bytes, z), &b = st.output(bytes, z_out);
    TRY(st.allocate());
    TRY(dojo_next_state_dev(s, a.p, b.p, nullptr));
    return st.finish();
}

int dojo_step_minimal(DojoHandle s, const void* x, const void* u, void* x_next, int32_t* status, int32_t* iters) {
    Enter enter_(s);
    if (!s || !x || !x_next) { g_err = "dojo_step_minimal: bad argument"; return DOJO_ERR_INVALID; }
    HIPCHK(hipSetDevice(s->device));
    const size_t B = s->B, w = s->w, nm = 2 * s->M.nu;
    const void* d_u = nullptr;
    ENSURE(s->d_x, B * (nm + 1) * w); ENSURE(s->d_xn, B * (nm + 1) * w);
    TRY(upload_step(s, s->d_x, x, nm, u, &d_u));
    TRY(dojo_step_minimal_dev(s, s->d_x, d_u, s->d_xn, s->d_status, s->d_iters, nullptr));
    s->have_grad = false;                                   // d_z / d_u now hold this (forward-only) step's inputs
    return download_step(s, x_next, s->d_xn, nm, status, iters);
}

int dojo_last_kernel_ms(DojoHandle s, double* ms) {
    Enter enter_(s);
    double a = 0, b = 0;
    int rc = dojo_last_kernel_times(s, &a, &b);
    if (rc == DOJO_OK && ms) *ms = a + b;
    return rc;
}

int dojo_last_kernel_times(DojoHandle s, double* step_ms, double* ift_ms) {
    Enter enter_(s);
    if (!s || !step_ms || !ift_ms || s->last_slot < 0) { g_err = "dojo_last_kernel_times: nothing was launched"; return DOJO_ERR_INVALID; }
    HIPCHK(hipSetDevice(s->device));
    DojoSim::Ev3& e = s->ring[s->last_slot];
    HIPCHK(hipEventSynchronize(e.b));
    float t = 0, t1 = 0;
    HIPCHK(hipEventElapsedTime(&t, e.a, e.b));
    if (e.has_mid) { HIPCHK(hipEventElapsedTime(&t1, e.a, e.m)); *step_ms = (double)t1; *ift_ms = (double)t - (double)t1; }
    else { *step_ms = (double)t / e.n; *ift_ms = 0.0; }
    return DOJO_OK;
}

int dojo_kernel_time_totals(DojoHandle s, double* step_ms, double* ift_ms, int64_t* launches, int32_t reset) {
    Enter enter_(s);
    if (!s) { g_err = "dojo_kernel_time_totals: bad argument"; return DOJO_ERR_INVALID; }
    HIPCHK(hipSetDevice(s->device));
    for (auto& e : s->ring) TRY(drain_slot(s, e));
    if (step_ms) *step_ms = s->acc_step_ms;
    if (ift_ms) *ift_ms = s->acc_ift_ms;
    if (launches) *launches = (int64_t)s->acc_n;
    if (reset) { s->acc_step_ms = s->acc_ift_ms = 0; s->acc_n = 0; }
    return DOJO_OK;
}

} // extern "C"
