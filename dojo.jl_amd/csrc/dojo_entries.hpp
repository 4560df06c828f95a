// dojo_entries.hpp -- what a kernel is built from around the lane program (dojo_device.hpp): the argument record, the LDS layout of a
// workgroup, the records that travel between the kernels (step -> IFT hand-off, factors) and the two per-lane entries.
// Shared by the HIP kernels (dojo_kernels.hip), the host that sizes the buffers (dojo_hip.hip) and the thread-based SIMT
// emulator (tests/emu).
#pragma once
#include "dojo_device.hpp"

namespace dj {

// ================================================================================================
// Kernel-level entry: one call per lane.
// ================================================================================================
// TIO = scalar type of the ABI buffers, T = state/residual precision (tables are stored in T)
template <class TIO, class T>
struct KernelArgs {
    typedef TIO io_type;
    Globals<T> G;
    const NodeP<T>* nodes;
    const ContactP<T>* contacts;
    int B;                       // number of environments
    const TIO* z;                  // [B,13Nb]
    const TIO* u;                  // [B,nu] or null
    const TIO* fext;               // [B,6Nb] or null          external force (world) and torque (body frame) per body
    TIO* z_next;                   // [B,13Nb]
    int* status;                 // [B] or null
    int* iters;                  // [B] or null
    TIO* vel;                      // [B,6Nb] or null          (v25, ω25)
    TIO* joint_imp;                // [B,n_joint_imp] or null  (get_solution order)
    TIO* contact_sg;               // [B,8Nc] or null          ([s; γ] per contact)
    TIO* dz;                       // [B][12Nb cols][12Nb rows] column-major per env, or null
    TIO* du;                       // [B][nu cols][12Nb rows] column-major per env, or null
    TIO* dc;                       // [B][5Nc cols][12Nb rows] contact-data Jacobian (get_contact_gradients), or null
    TIO* res;                      // [B,6Nb] or null          body residual rows at the solution (for the Storage kernel)
    T* sol;                        // [B][S][HandOff<MAXC>::size] converged solution in state precision: step kernel -> IFT kernel (or null)
    T* fac;                        // [workgroups][FAC_PER_LANE][lanes] quad mapping: the final supernode factors of every lane (explicit inverses; or null: nobody reads them)
    T* lu = nullptr;               // [workgroups][dj::LU_PER_LANE][lanes] quad mapping: the IFT kernel's own LU-form factors between its phases (or null)
    T* blk = nullptr;              // [workgroups][90][lanes] quad mapping: un-factored supernode rows of refining environments (DJ_REFINE; or null)
    long long ypark_stride = 0;    // elements per workgroup of ypark
    T* ypark = nullptr;            // [workgroups][batches][6][3][lanes / 2] quad mapping, ABI type narrower than the arithmetic: the IFT's forward-substituted
                                   // right-hand sides in full precision between the two sweeps (or null: they wait in the output buffer, in the ABI type)
    T* msg = nullptr;              // [B][level-1 supernodes][batches][2 roles][18] quad mapping: what the children of a root post to its body rows during the
    long long msg_stride = 0;      // up-sweep (read back by the root phase, gradient_columns_quad); msg_stride = elements per environment
    int* flag = nullptr;           // [B] 1: the plain step kernel deferred this environment to the refining kernels (DJ_REFINE; or null)
    T* mu_out = nullptr;           // [B] or null: mechanism.μ when mehrotra! returned (src/solver/mehrotra.jl:45), fp64
    T* diag_out = nullptr;         // [B][2] or null: diagnostics of the final linearization: max γ/s of the cones, largest Gauss-Jordan multiplier
    const TraSD<T>* tsd = nullptr; // [Nb + 1] translational springs / dampers per supernode, or null (read by the DJ_TSD builds only)
    const MLimP<T>* mlim = nullptr;// [Nb + 1] limits on several coordinates per supernode, or null (read by the DJ_MLIM builds only)
    const NodeP<T>* cuts = nullptr;// [ncut] loop-closing joints (read by the DJ_CUT builds only): the joint fields of NodeP, parent = body a, child[0] = body b
    int ncut = 0;
    T* cutws = nullptr;            // [B][CUTWS] workspace of the cut elements (M_c, H, the factored small system), or null
    // iteration cap + continuation (Globals::iter_cap > 0; all three set or all null):
    T* resume = nullptr;           // [B][CARRY_PER_ENV] solver scalars of the environments the step kernel left unfinished (DJ_STATUS_CONTINUE);
                                   // entry CARRY_MARK: 1 for the environments of a workgroup on the continuation list, 0 for the others (written by
                                   // the step kernel for every environment, never by the continuation: the IFT kernel of the others runs next to it)
    int* cont_list = nullptr;      // [workgroups of this launch] workgroup indices with an unfinished environment, in the order they finished
    int* cont_count = nullptr;     // [1] entries of cont_list (zeroed before the step kernel, atomically advanced by it)
    int wave_base = 0;             // index of this launch's first workgroup in the batch: cont_list holds batch-level workgroup indices (the
                                   // continuation kernels run once over the whole batch, behind the step kernels of all environment groups)
    const int* dispatch = nullptr; // [workgroups of this launch] the step kernel's hardware workgroup -> workgroup of this launch it works for (a permutation:
                                   // the longest solves of the previous step first, dojo_set_dispatch_order), or null: in order
#ifdef DJ_DEBUG
    T* dbg = nullptr;            // [B][Nb][512] test hook
#endif
};

// LDS layout of one workgroup (= one wavefront, or NW wavefronts for mechanisms of 17..32 bodies) in the quad mapping.
// LOCKSTEP (the GPU): everything the four lanes of a supernode hold identically exists once per supernode in LDS; the
// four lanes read it with broadcast ds_reads and write identical values in the same instruction.  The SIMT emulator's
// threads are not in lock step, so there NodeP / Lane stay per-lane and Cold is per-lane in "LDS".
//   phase A (Newton loop; data blocks of the IFT):
//     [NodeP x NSN][Lane x NSN][Cold x NSN (or per lane)][ContactCold pool][mailbox (step kernel)]
//   IFT column sweeps (overlay from offset 0: NodeP / Lane / Cold are dead by then, the few NodeP fields the sweeps
//   need are cached in registers):
//     [QuadRhs x NSN][mailbox]
//   [reduction scratch, 64 B] at the end
template <class T, int MAXC>
struct LaneSlot { Lane<T, MAXC> L; T pad_[(sizeof(Lane<T, MAXC>) / sizeof(T)) % 2 == 0 ? 1 : 2]; };   // odd stride in 8-byte words
constexpr int lds_imax(int a, int b) { return a > b ? a : b; }
// GRAD: 0 = step kernel, 1 = IFT kernel (state + control columns), 2 = IFT kernel for the contact-data columns
template <class TIO, class T, int MAXC, int GRAD, bool QUAD, bool LOCKSTEP, int NW = 1>
struct StepLds {
    static constexpr int NSN = 16 * NW;                                                     // supernode slots of the workgroup
    static constexpr bool share = QUAD && LOCKSTEP;
    static constexpr int node_bytes = share ? (int)sizeof(NodeSlot<T>) * NSN : 0;
    static constexpr int lane_off = node_bytes;
    static constexpr int lane_bytes = node_bytes + (share ? (int)sizeof(LaneSlot<T, MAXC>) * NSN : 0);   // end of the Lane block
    static constexpr int cold_n = LOCKSTEP ? NSN : 64 * NW;
    static constexpr bool cold_in_lds = QUAD;
    static constexpr int cold_off = lane_bytes;
    static constexpr int cold_bytes = QUAD ? (int)sizeof(Cold<T, MAXC>) * cold_n : 0;
    // contact rows: one slot per (supernode, contact) for a single-wave workgroup, one slot per contact of the
    // environment (at most 16) for NW > 1 -- there the per-supernode array would not fit
    static constexpr bool pool_by_id = NW > 1;
    static constexpr int pool_n = !QUAD ? 0 : (pool_by_id ? 16 : cold_n * MAXC);
    static constexpr int pool_off = cold_off + cold_bytes;
    static constexpr int pool_bytes = (int)sizeof(ContactCold<T>) * pool_n;
    // Newton step and the iterate at the start of the line search, once per supernode (step kernel, when there is room:
    // frees ~100 registers during the residual evaluations of the line search)
    static constexpr int ls_slot = (int)((sizeof(Step<T, MAXC>) + sizeof(SolSnap<T, MAXC>)) / 8 + (((sizeof(Step<T, MAXC>) + sizeof(SolSnap<T, MAXC>)) / 8) % 2 == 0 ? 1 : 0)) * 8;
    static constexpr bool ls_in_lds = share && !GRAD && NW == 1 && MAXC == 1;                 // (must match LaneProgram::kLsInLds)
    static constexpr int ls_off = pool_off + pool_bytes;
    static constexpr int a_end = ls_off + (ls_in_lds ? ls_slot * NSN : 0);
    static constexpr int rhs_bytes = !QUAD ? 0 : GRAD == 1 ? (int)sizeof(QuadRhs<TIO>) * NSN : GRAD == 2 ? (int)sizeof(ConRhs<MAXC>) * NSN : 0;
    static constexpr int mail_need = QUAD ? 2 * NSN * 20 * 8 : 0;
    static constexpr int rhs_off = 0;
    // (contact-data kernel: the mailbox keeps its own room behind the phase-A data; packed right behind the ConRhs blocks
    //  the last supernode's block read back zeros on the GPU -- not understood, the kernel is not LDS-critical)
    // (IFT kernel: behind both the phase-A data and the right-hand sides -- a workgroup that factors its own LU form
    //  (gradients) evaluates the linearization, which uses the mailbox while NodeP / Lane / Cold / the contact rows are alive)
    static constexpr int mail_off = (QUAD && GRAD == 2) ? a_end : (QUAD && GRAD) ? lds_imax(a_end, rhs_off + rhs_bytes) : a_end;
    static constexpr int red_off = lds_imax(a_end, mail_off + mail_need);
    static constexpr int qred_off = red_off + 64;                    // per-supernode values of the environment reductions (3 at a time)
    static constexpr int info_off = qred_off + (QUAD ? 3 * NSN * 8 : 0);   // SweepInfo per supernode (IFT kernels)
    static constexpr int info_end = info_off + ((QUAD && GRAD) ? NSN * (int)sizeof(SweepInfo) : 0);
    // Staging areas of the row-layout level passes (LaneProgram::factorize_rows; step kernels of the single-wavefront quad mapping with one
    // contact per body): A = 4 supernodes x 12 rows of S (stride ROW_RS doubles: odd, so that the 32 lanes of a ds_read_b64 group hit 32
    // bank pairs), later their 6 rows of L and of Dup; B = their 12 rows of U (stride ROW_US).  On the GPU A lies over the Newton step /
    // line-search base, which are dead between the line search and the next solve; B takes what is left of the 40 KB a workgroup may
    // use with four workgroups per CU.
    static constexpr int ROW_RS = 13, ROW_US = 7;
    static constexpr bool rows = QUAD && GRAD == 0 && ((NW == 1 && MAXC == 1) || NW == 2);    // (two wavefronts: staging areas per wavefront, behind the layout)
    static constexpr int stA_bytes = NW * 4 * 12 * ROW_RS * 8, stB_bytes = NW * 4 * 12 * ROW_US * 8;
    static_assert(4 * 6 * (ROW_RS + ROW_US) * 8 <= stA_bytes / NW, "L and Dup rows reuse area A");
    static constexpr int stA_off = !rows ? 0 : ls_in_lds ? ls_off : info_end;
    static constexpr int stB_off = !rows ? 0 : ls_in_lds ? info_end : info_end + stA_bytes;
    static_assert(!rows || !ls_in_lds || ls_slot * NSN >= stA_bytes, "area A must fit the line-search block it overlays");
    // ... and of the IFT kernel's LU-form passes (LaneProgram::factorize_rows_lu; GRAD == 1): A = the S rows in and the factor rows out (stride
    // LU_RS), the rows of L in and of m out over its first half; B = the rows of U in / T out (stride ROW_US) and of Dup in (stride LU_DS).  B
    // lies where the right-hand-side blocks reach beyond the phase-A data -- nothing of them is alive while the linearization is factored --
    // when that stretch is long enough (fp32 ABI: exactly), A behind everything else: 40 768 of the 40 960 bytes of four workgroups per CU.
    static constexpr int LU_RS = 12, LU_DS = 6;
    static constexpr bool rows_lu = QUAD && NW == 1 && MAXC == 1 && GRAD == 1;
    static constexpr int luA_bytes = 4 * 12 * LU_RS * 8, luB_bytes = 4 * 12 * ROW_US * 8 + 4 * 6 * LU_DS * 8;
    static constexpr bool luB_in_rhs = rows_lu && (rhs_off + rhs_bytes - a_end >= luB_bytes) && (mail_off >= a_end + luB_bytes);
    static constexpr int luA_off = info_end;
    static constexpr int luB_off = luB_in_rhs ? a_end : info_end + luA_bytes;
    static constexpr int bytes = rows ? stB_off + stB_bytes : rows_lu ? (luB_in_rhs ? info_end + luA_bytes : info_end + luA_bytes + luB_bytes) : info_end;
};
template <class TIO, class T, int MAXC, int GRAD, bool QUAD, bool LOCKSTEP = true, int NW = 1>
constexpr int step_lds_bytes() { return StepLds<TIO, T, MAXC, GRAD, QUAD, LOCKSTEP, NW>::bytes; }

// The step -> IFT hand-off record (KernelArgs::sol), one per supernode, in the state precision: the iterate -- v ω λ(6), s,γ of the
// joint limit, s,γ of the contacts, μ -- and the pieces of the final linearization the IFT needs besides the factors: t_a, t_b (limit
// condensation), G134.  The layout is stated here and nowhere else (DESIGN.md §2 has it as a table).  It is plain constexpr data on purpose:
// the entries index with `HO::cone_s + HO::per_contact * c + i`, which folds in the front end; offsets or stores / restores behind a function,
// even a forced-inline one, moved the register allocation of some build ("Kernel entries").
// NOTE: a step that skips the linearization after its converging iteration (need_factors = false: every launch without the refining
// kernels) leaves t_a / t_b / G134 -- and KernelArgs::diag_out -- at the LAST linearization it did perform, i.e. one iterate back; the plain
// IFT kernel never reads them (lu_prepare() evaluates the linearization at the restored solution before any use), the refining one
// re-evaluates them too (grad_entry MODE 2).  They travel for the explicit-inverse consumers only.
// (GEN: the general lane-mapping builds -- DJ_MLIM and DJ_CUT together -- append (s_up, s_lo, γ_up, γ_lo) of up to six limited coordinates and the multipliers
//  of the cut joints; the host sizes the buffer with GEN = true for mechanisms that take those builds)
static_assert((DJ_MLIM != 0) == (DJ_CUT != 0), "the general lane-mapping builds carry DJ_MLIM and DJ_CUT together");
template <int MAXC, bool GEN = (DJ_MLIM != 0)>
struct HandOff {
    static constexpr int v = 0, w = 3, lam = 6;
    static constexpr int lim_s = 12, lim_s_lo = 13, lim_g = 14, lim_g_lo = 15;  // the joint limit: s_up, s_lo, γ_up, γ_lo
    static constexpr int cone_s = 16, cone_g = 20, per_contact = 8;            // contact c: s(4) at cone_s + per_contact c, γ(4) at cone_g + per_contact c
    static constexpr int mu = cone_s + per_contact * MAXC, t_a = mu + 1, t_b = t_a + 6;
    static constexpr int G134 = t_b + 6, per_G134 = 18;                        // contact c: 18 values at G134 + per_G134 c
    static constexpr int mlim = G134 + per_G134 * MAXC, mlim_g = 2, per_mlim = 4;   // GEN: limited coordinate m < NLM_GEN: (s_up, s_lo) at mlim + per_mlim m, (γ_up, γ_lo) mlim_g further
    static constexpr int cut = mlim + per_mlim * NLM_GEN, per_cut = 6;               // GEN: the six multipliers of cut joint c < NCUT at cut + per_cut c
    static constexpr int flag = GEN ? cut + per_cut * NCUT : mlim;             // 1.0 if the environment's solves were being refined (DJ_REFINE)
    static constexpr int size = flag + 1;
};
template <int MAXC, bool GEN> constexpr bool hand_off_ok() {      // the closed form the layout has had since the general builds joined
    return HandOff<MAXC, GEN>::size == 6 + 6 + 4 + 8 * MAXC + 1 + 12 + 18 * MAXC + (GEN ? 24 + 6 * NCUT : 0) + 1 && HandOff<MAXC, GEN>::flag == HandOff<MAXC, GEN>::size - 1;
}
static_assert(hand_off_ok<1, false>() && hand_off_ok<4, false>() && hand_off_ok<8, false>() && hand_off_ok<1, true>() && hand_off_ok<4, true>() && hand_off_ok<8, true>(), "hand-off record layout");
constexpr int HANDOFF_MAX = HandOff<8, true>::size;     // the largest record of any build: the host sizes one buffer for all of them
// doubles per supernode of the record: what the emulator (tests/emu) sizes its KernelArgs::sol buffer with
template <int MAXC, bool GEN = (DJ_MLIM != 0)> constexpr int sol_record() { return HandOff<MAXC, GEN>::size; }

// quad mapping: the factors themselves travel too (KernelArgs::fac): rows 3q..3q+2 of S⁻¹ (36 values) and of U (18), columns 3q..3q+2
// of L (18) per lane, stored [workgroup][FAC_PER_LANE][lanes of the workgroup]: coalesced
constexpr int FAC_S = 0, FAC_U = 36, FAC_L = 54, FAC_PER_LANE = 72;

// The forward step and the IFT gradients are separate kernels (separate register allocations: the
// gradient sweeps must not cost the Newton loop its registers).  The IFT kernel rebuilds the lane
// program from (z, u), restores the converged solution from the hand-off record and re-linearizes
// there -- the same final linearization mehrotra! leaves behind (src/gradients/state.jl:78-84).
#if DJ_CUT
#define DJ_CUT_SETUP if constexpr (!QUAD) { prog.cutp = A.cuts; prog.ncut = (A.cuts && A.cutws) ? A.ncut : 0;                                              \
        prog.cws = A.cutws ? A.cutws + (size_t)(env < A.B ? env : 0) * CUTWS : nullptr;                                                             \
        for (int c_ = 0; c_ < NCUT; ++c_) for (int i = 0; i < 6; ++i)                                                                                \
            prog.cue[c_][i] = (has_u && c_ < prog.ncut && env < A.B && i < A.cuts[c_].nu_t + A.cuts[c_].nu_r) ? T(A.u[(size_t)env * G.nu + A.cuts[c_].u_off + i]) : T(0); \
        prog.cut_begin(); }
#else
#define DJ_CUT_SETUP
#endif
#if DJ_TSD && DJ_MLIM
#define DJ_TSD_SETUP prog.tsd = A.tsd ? A.tsd + (k < G.Nb ? k : G.Nb) : nullptr; prog.tlim = prog.tsd != nullptr && prog.tsd->nlim > 0; prog.mlp = A.mlim ? A.mlim + (k < G.Nb ? k : G.Nb) : nullptr;
#elif DJ_TSD
#define DJ_TSD_SETUP prog.tsd = A.tsd ? A.tsd + (k < G.Nb ? k : G.Nb) : nullptr; prog.tlim = prog.tsd != nullptr && prog.tsd->nlim > 0;
#elif DJ_MLIM
#define DJ_TSD_SETUP prog.mlp = A.mlim ? A.mlim + (k < G.Nb ? k : G.Nb) : nullptr;
#else
#define DJ_TSD_SETUP
#endif
#ifdef DJ_PROF2
#define DJ_P2_SETUP { prog.p2c = (unsigned long long*)wv.p2_; wv.sync(); if (lane < 24) prog.p2c[lane] = 0ull; wv.sync(); }
#else
#define DJ_P2_SETUP
#endif
#define DJ_LANE_SETUP(GRAD_LAYOUT, ENV_OK)                                                                                \
    const Globals<T>& G = A.G;                                                                                            \
    const int stride = QUAD ? 4 : 1;                                                                                      \
    const int envl = stride * G.S, E = wv.width() / envl;        /* lanes per environment, environments per workgroup */  \
    const int lane = wv.lane();                                                                                           \
    const int slot = lane / envl, k = (lane % envl) / stride, q = lane % stride;                                          \
    const int env = wave_index * E + slot;                                                                                \
    const bool active = (env < A.B) && (k < G.Nb) && (ENV_OK);                                                            \
    const int base = slot * envl;                                                                                         \
    typedef StepLds<TIO, T, MAXC, (GRAD_LAYOUT), QUAD, Wave::kLockstep, Wave::kWaves> LY;                                   \
    constexpr bool SHARE = QUAD && Wave::kLockstep;                                                                       \
    char* lds = (char*)wv.lds();                                                                                          \
    const NodeP<T>& Pg = A.nodes[k < G.Nb ? k : G.Nb];         /* idle supernode slots: the table's extra entry (node 0 without contacts) */ \
    if (SHARE) ((NodeSlot<T>*)lds)[lane / 4].P = Pg;           /* the four lanes store identical values */                \
    const NodeP<T>& P = SHARE ? ((NodeSlot<T>*)lds)[lane / 4].P : Pg;                                                     \
    Lane<T, MAXC> lane_local;                                                                                             \
    Cold<T, MAXC> cold_local;                                                                                             \
    ContactCold<T> pool_local[QUAD ? 1 : MAXC];                                                                           \
    Lane<T, MAXC>& lane_state = SHARE ? ((LaneSlot<T, MAXC>*)(lds + LY::lane_off))[lane / 4].L : lane_local;             \
    Cold<T, MAXC>& cold = LY::cold_in_lds ? ((Cold<T, MAXC>*)(lds + LY::cold_off))[SHARE ? lane / 4 : lane] : cold_local; \
    LaneProgram<T, TL, MAXC, QUAD, Wave> prog(wv, G, P, A.contacts, base, k, q, active, lane_state, cold);                \
    if (QUAD) {                                                                                                           \
        prog.cpool = (ContactCold<T>*)(lds + LY::pool_off); prog.pool_by_id = LY::pool_by_id;                             \
        prog.pool_base = LY::pool_by_id ? 0 : (SHARE ? lane / 4 : lane) * MAXC;                                           \
        prog.gb_lds = ((GRAD_LAYOUT) == 2) ? (void*)(((ConRhs<MAXC>*)(lds + LY::rhs_off)) + lane / 4) : (void*)(((QuadRhs<TIO>*)lds) + lane / 4); \
        prog.mail = (double*)(lds + LY::mail_off); prog.chpack_init();                                                    \
        DJ_P2_SETUP                                                                                                       \
        prog.qred = (double*)(lds + LY::qred_off);                                                                        \
        if (GRAD_LAYOUT) prog.sinfo = (SweepInfo*)(lds + LY::info_off);                                                   \
        if (A.msg) prog.msg = DJ_GLOBAL_PTR(T, A.msg) + (size_t)(env < A.B ? env : 0) * (size_t)A.msg_stride;                 \
        if (LY::ls_in_lds) prog.ls_lds = lds + LY::ls_off + (size_t)(lane / 4) * LY::ls_slot;                              \
        prog.rows_here = LY::rows || LY::rows_lu;                                                                         \
        if (LY::rows) { prog.stA = (double*)(lds + LY::stA_off); prog.stB = (double*)(lds + LY::stB_off); prog.rows_init(); }  \
        if (LY::rows_lu) { prog.stA = (double*)(lds + LY::luA_off); prog.stB = (double*)(lds + LY::luB_off); prog.rows_init(); } \
        if (SHARE) { prog.lane_slots = lds + LY::lane_off; prog.lane_slot_stride = (int)sizeof(LaneSlot<T, MAXC>); }              \
        if (A.lu) { prog.lu = DJ_GLOBAL_PTR(T, A.lu) + (size_t)wave_index * LU_PER_LANE * wv.width() + lane; prog.lu_stride = wv.width(); }                \
        if (A.blk) { prog.blk = DJ_GLOBAL_PTR(T, A.blk) + (size_t)wave_index * 90 * wv.width() + lane; prog.blk_stride = wv.width(); }     \
        if (A.ypark) prog.ypark = DJ_GLOBAL_PTR(T, A.ypark) + (size_t)wave_index * (size_t)A.ypark_stride + lane;                                \
    } else { prog.cpool = pool_local; prog.pool_by_id = false; prog.pool_base = 0; }                                      \
    DJ_TSD_SETUP                                                                                                          \
    T zb[13], ue[6] = {0, 0, 0, 0, 0, 0};                                                                                 \
    for (int i = 0; i < 13; ++i) zb[i] = active ? T(A.z[(size_t)env * 13 * G.Nb + 13 * k + i]) : T(0);                   \
    if (sizeof(TIO) < sizeof(T) && active) {   /* a narrower ABI type cannot hold a unit quaternion: the state it stands for is (x, v, q/|q|, ω) */ \
        const T iq_ = trcp(tsqrt(zb[6] * zb[6] + zb[7] * zb[7] + zb[8] * zb[8] + zb[9] * zb[9]));                         \
        for (int i = 6; i < 10; ++i) zb[i] *= iq_;                                                                        \
    }                                                                                                                     \
    const bool has_u = A.u != nullptr;                                                                                    \
    if (active && has_u) for (int i = 0; i < 6; ++i) if (i < P.nu_t + P.nu_r) ue[i] = T(A.u[(size_t)env * G.nu + P.u_off + i]); \
    T fe[6] = {0, 0, 0, 0, 0, 0};                                                                                         \
    const bool has_f = A.fext != nullptr;                                                                                 \
    if (active && has_f) for (int i = 0; i < 6; ++i) fe[i] = T(A.fext[(size_t)env * 6 * G.Nb + 6 * k + i]);             \
    prog.begin_step(zb, has_u ? ue : nullptr, has_f ? fe : nullptr);                                                        \
    DJ_CUT_SETUP

// IFT kernel entry: one call per lane
// MODE 0: state + control columns, pipelined sweeps; 1: contact-data columns; 2: state + control columns of the environments
// whose solves were being refined, column by column through the refined general solve (LDS layout of the step kernel:
// NodeP / Lane / Cold stay alive)
// CONT (MODE 0, iteration cap): false = the environments the step kernel finished itself (all of them without a cap), true = `wave_index`
// comes from the continuation list and the environments the continuation kernel finished are served
template <class TIO, class T, class TL, int MAXC, bool QUAD, class Wave, int MODE = 0, bool CONT = false>
DJ_HD void grad_entry(Wave& wv, const KernelArgs<TIO, T>& A, int wave_index) {
    static_assert(!CONT || MODE == 0, "continuation lists exist for the plain IFT kernel only");
    typedef HandOff<MAXC> HO;
    if constexpr (QUAD && MODE == 0) {
        if (A.resume != nullptr) {                              // (uniform) a workgroup without an environment of this launch's kind leaves at once
            const int stride_ = 4, envl_ = stride_ * A.G.S, E_ = wv.width() / envl_, lane_ = wv.lane();
            const int env_ = wave_index * E_ + lane_ / envl_, k_ = (lane_ % envl_) / stride_;
            const bool act_ = (env_ < A.B) && (k_ < A.G.Nb);
            if (!wv.any(act_ && (A.resume[(size_t)env_ * CARRY_PER_ENV + CARRY_MARK] != T(0)) == CONT)) return;
        }
    }
    if constexpr (QUAD && DJ_REFINE && (MODE == 0 || MODE == 2)) {
        // refined environments belong to the MODE 2 kernel; a workgroup without work for this kernel leaves at once (uniform)
        const int stride_ = 4, envl_ = stride_ * A.G.S, E_ = wv.width() / envl_, lane_ = wv.lane();
        const int env_ = wave_index * E_ + lane_ / envl_, k_ = (lane_ % envl_) / stride_;
        const bool act_ = (env_ < A.B) && (k_ < A.G.Nb);
        const bool fl_ = act_ && A.sol[((size_t)env_ * A.G.S + (size_t)k_) * HO::size + HO::flag] != T(0);
        if (MODE == 0 ? !wv.any(act_ && !fl_) : !wv.any(fl_)) return;
    }
    static_assert(MODE != 2 || Wave::kRefine || !(QUAD && DJ_REFINE), "the MODE 2 IFT kernel needs a refining Wave");
    // (MODE 2 is gated per environment, by the flag of its supernode 0: wave-uniform over the environment's lanes)
    DJ_LANE_SETUP(MODE == 0 ? 1 : MODE == 1 ? 2 : 0,
                  MODE == 2 ? A.sol[(size_t)env * G.S * HO::size + HO::flag] != T(0)
                            : (MODE != 0 || !QUAD || A.resume == nullptr || (A.resume[(size_t)env * CARRY_PER_ENV + CARRY_MARK] != T(0)) == CONT))
    bool flagged = false;
    {   // restore the converged solution (identical on the four lanes of a quad)
        const T* r = A.sol + ((size_t)env * G.S + (size_t)k) * HO::size;
        if (active) {
            flagged = r[HO::flag] != T(0);
            for (int i = 0; i < 3; ++i) { prog.L.v[i] = r[HO::v + i]; prog.L.w[i] = r[HO::w + i]; }
            for (int i = 0; i < 6; ++i) prog.L.lam[i] = r[HO::lam + i];
            prog.L.ls[0] = r[HO::lim_s]; prog.L.ls[1] = r[HO::lim_s_lo]; prog.L.lg[0] = r[HO::lim_g]; prog.L.lg[1] = r[HO::lim_g_lo];
#pragma unroll
            for (int c = 0; c < MAXC; ++c) for (int i = 0; i < 4; ++i) { prog.L.cs[c][i] = r[HO::cone_s + HO::per_contact * c + i]; prog.L.cg[c][i] = r[HO::cone_g + HO::per_contact * c + i]; }
            prog.mu = r[HO::mu];
#if DJ_MLIM
            for (int m = 0; m < NLM; ++m) for (int i = 0; i < 2; ++i) { prog.L.mls[m][i] = r[HO::mlim + HO::per_mlim * m + i]; prog.L.mlg[m][i] = r[HO::mlim + HO::per_mlim * m + HO::mlim_g + i]; }
#endif
#if DJ_CUT
            for (int c = 0; c < NCUT; ++c) for (int i = 0; i < 6; ++i) prog.clam[c][i] = r[HO::cut + HO::per_cut * c + i];
#endif
            if (QUAD) {                                        // ... and the pieces of the final linearization
                for (int i = 0; i < 6; ++i) { prog.F.t_a[i] = r[HO::t_a + i]; prog.F.t_b[i] = r[HO::t_b + i]; }
#pragma unroll
                for (int c = 0; c < MAXC; ++c) if (c < P.ncontact) for (int i = 0; i < 18; ++i) prog.ccold(c).G134[i] = r[HO::G134 + HO::per_G134 * c + i];
            }
        }
    }
#ifdef DJ_PROF
    unsigned long long t_all = wv.clock();
#endif
    if constexpr (QUAD) { if (A.fac != nullptr) {              // the final factors of the Newton loop, as the step kernel left them (uniform)
        const T* f = A.fac + (size_t)wave_index * FAC_PER_LANE * wv.width() + lane;
        const int W = wv.width();
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 12; ++j) prog.F.Sq[i][j] = TL(f[(size_t)(FAC_S + 12 * i + j) * W]);
#pragma unroll
            for (int j = 0; j < 6; ++j) { prog.F.Uq[i][j] = TL(f[(size_t)(FAC_U + 6 * i + j) * W]); prog.F.Lq[j][i] = TL(f[(size_t)(FAC_L + 6 * i + j) * W]); }
        }
    } } else {
        prog.linearize();                                     // lane mapping: rebuild the final linearization instead
    }
    if constexpr (MODE == 0) prog.gradients(A, env);
    else if constexpr (MODE == 2) {
        if constexpr (QUAD && DJ_REFINE) {
            // the un-factored rows of the final linearization (the step kernel's copy may be older than its last iterate's):
            // set_entries! once more into scratch rows; this also restores C134 / G134 and the limit rows of F
            TL S2[3][12], U2[3][6], L2[6][3];
            QuadBlocks<TL> K2(S2, U2, L2, q);
            prog.refine = flagged;
            prog.template evaluate<true>(K2);
            prog.condense_limits(K2);
            prog.store_blocks(K2);
            prog.template gradients<true>(A, env, flagged);
        }
    }
    else if constexpr (QUAD) prog.gradients_contact(A, env);
#ifdef DJ_PROF2
    if (active && q == 0 && A.vel && k == 8) { TIO* vo = A.vel + (size_t)env * 6 * G.Nb + 48; for (int i = 0; i < 16; ++i) vo[i] = TIO((double)prog.p2c[i]); }
#endif
#ifdef DJ_PROF
    if (active && q == 0 && A.vel && k == 2) { TIO* vo = A.vel + (size_t)env * 6 * G.Nb + 12; vo[0] = TIO((double)prog.pc[0]); vo[1] = TIO((double)prog.pc[1]); vo[2] = TIO((double)prog.pc[5]); vo[3] = TIO((double)prog.pc[6]); vo[4] = TIO((double)(wv.clock() - t_all)); vo[5] = TIO((double)prog.pc[4]); vo[6] = TIO((double)prog.pc[2]); vo[7] = TIO((double)prog.pc[3]); vo[8] = TIO((double)prog.pc[7]); }
#endif
}

// CONT = true: the continuation kernel's entry (Globals::iter_cap): `wave_index` is a workgroup of the step kernel that left
// environments unfinished (DJ_STATUS_CONTINUE in KernelArgs::status); their iterate comes back from the hand-off record, the
// loop scalars from KernelArgs::resume, and the Newton loop goes on.  The other environments of the workgroup stay as they are.
template <class TIO, class T, class TL, int MAXC, bool QUAD, class Wave, bool CONT = false>
DJ_HD void step_entry(Wave& wv, const KernelArgs<TIO, T>& A, int wave_index) {
    constexpr bool RF = QUAD && DJ_REFINE && Wave::kRefine;      // the refining build: re-solves the environments the plain kernel deferred
    static_assert(!(RF && CONT), "the continuation kernel is a plain build");
    typedef HandOff<MAXC> HO;
    if constexpr (RF) {
        const int envl_ = 4 * A.G.S, E_ = wv.width() / envl_, env_ = wave_index * E_ + wv.lane() / envl_;
        if (A.flag == nullptr || !wv.any(env_ < A.B && A.flag[env_] != 0)) return;          // nothing deferred in this workgroup (uniform)
    }
    DJ_LANE_SETUP(0, CONT ? A.status[env] == DJ_STATUS_CONTINUE : (!RF || A.flag[env] != 0))
#ifdef DJ_DEBUG
    prog.dbg_on = A.dbg != nullptr; prog.trace = getenv("DJ_TRACE") != nullptr;
    if (A.dbg && active && q == 0) prog.dbg = A.dbg + ((size_t)env * G.Nb + k) * 512;
#endif
    int iters = 0;
#ifdef DJ_PROF
    unsigned long long t_all = wv.clock();
#endif
    int status;
    if constexpr (CONT) {
        SolveCarry<T> carry;
        carry.undercut = G.undercut; carry.rvio = carry.bvio = T(0); carry.n = 0; carry.no_progress = 0; carry.excessive = 0;
        if (active) {                                          // the iterate the capped solve stopped at (identical on the four lanes of a quad)
            const T* r = A.sol + ((size_t)env * G.S + (size_t)k) * HO::size;
            for (int i = 0; i < 3; ++i) { prog.L.v[i] = r[HO::v + i]; prog.L.w[i] = r[HO::w + i]; }
            for (int i = 0; i < 6; ++i) prog.L.lam[i] = r[HO::lam + i];
            prog.L.ls[0] = r[HO::lim_s]; prog.L.ls[1] = r[HO::lim_s_lo]; prog.L.lg[0] = r[HO::lim_g]; prog.L.lg[1] = r[HO::lim_g_lo];
#pragma unroll
            for (int c = 0; c < MAXC; ++c) for (int i = 0; i < 4; ++i) { prog.L.cs[c][i] = r[HO::cone_s + HO::per_contact * c + i]; prog.L.cg[c][i] = r[HO::cone_g + HO::per_contact * c + i]; }
            prog.mu = r[HO::mu];
            const T* cr = A.resume + (size_t)env * CARRY_PER_ENV;
            carry.undercut = cr[CARRY_UNDERCUT]; carry.rvio = cr[CARRY_RVIO]; carry.bvio = cr[CARRY_BVIO];
            carry.n = (int)cr[CARRY_N]; carry.no_progress = (int)cr[CARRY_NO_PROGRESS]; carry.excessive = (int)cr[CARRY_EXCESSIVE];
        }
        carry.n = G.iter_cap;                                  // (wave-uniform: the capped loop leaves at exactly this iteration)
        status = prog.template mehrotra<true>(iters, /*need_factors=*/false, &carry);
    } else {
    // The factors of the final linearization leave this kernel only through A.fac (the refining IFT kernel reads them); the plain IFT
    // kernels linearize once more themselves (lu_prepare / linearize in grad_entry), so a differentiable step without refinement may
    // skip the set_entries! + factorization after the converging iteration exactly like a forward-only one.
    status = prog.mehrotra(iters, /*need_factors=*/QUAD && A.fac != nullptr, nullptr,
                           (!RF && G.iter_cap > 0 && A.resume != nullptr) ? DJ_GLOBAL_PTR(T, A.resume) + (size_t)(env < A.B ? env : 0) * CARRY_PER_ENV : nullptr);
    }
#ifdef DJ_PROF
    prog.pc[7] = wv.clock() - t_all;
#endif
    if constexpr (!RF && !CONT) {                             // iteration cap: the loop scalars of the unfinished solves, and this workgroup on the continuation list
        if (A.resume != nullptr) {
            // (the mark is per WORKGROUP: the IFT of a listed workgroup's finished environments waits for the continuation as well, so that
            //  no IFT launch ever works on part of a workgroup -- the per-lane staging areas KernelArgs::lu / ypark are indexed by workgroup)
            const bool listed = wv.any(active && status == DJ_STATUS_CONTINUE);
            if (active && q == 0 && k == 0) A.resume[(size_t)env * CARRY_PER_ENV + CARRY_MARK] = listed ? T(1) : T(0);
            if (listed && lane == 0) A.cont_list[wv.atomic_inc(A.cont_count)] = A.wave_base + wave_index;
        }
    }
    if constexpr (CONT) { if (Wave::kReplicas > 1 && wv.replica() != 0) return; }   // every replica holds the same result; the first one writes it
    T gr_env = T(0);
    if constexpr (QUAD && DJ_REFINE) { if (A.diag_out) { T v1[1] = {prog.growth}; prog.template env_reduce_quad_all<1>(v1); gr_env = v1[0]; } }
    if (active && q == 0 && A.sol) {                          // hand-off to the IFT kernel, in the state precision
        T* r = A.sol + ((size_t)env * G.S + (size_t)k) * HO::size;
        for (int i = 0; i < 3; ++i) { r[HO::v + i] = prog.L.v[i]; r[HO::w + i] = prog.L.w[i]; }
        for (int i = 0; i < 6; ++i) r[HO::lam + i] = prog.L.lam[i];
        r[HO::lim_s] = prog.L.ls[0]; r[HO::lim_s_lo] = prog.L.ls[1]; r[HO::lim_g] = prog.L.lg[0]; r[HO::lim_g_lo] = prog.L.lg[1];
#pragma unroll
        for (int c = 0; c < MAXC; ++c) for (int i = 0; i < 4; ++i) { r[HO::cone_s + HO::per_contact * c + i] = prog.L.cs[c][i]; r[HO::cone_g + HO::per_contact * c + i] = prog.L.cg[c][i]; }
        r[HO::mu] = prog.mu;
#if DJ_MLIM
        for (int m = 0; m < NLM; ++m) for (int i = 0; i < 2; ++i) { r[HO::mlim + HO::per_mlim * m + i] = prog.L.mls[m][i]; r[HO::mlim + HO::per_mlim * m + HO::mlim_g + i] = prog.L.mlg[m][i]; }
#endif
#if DJ_CUT
        for (int c = 0; c < NCUT; ++c) for (int i = 0; i < 6; ++i) r[HO::cut + HO::per_cut * c + i] = prog.clam[c][i];
#endif
        if (QUAD) {
            for (int i = 0; i < 6; ++i) { r[HO::t_a + i] = prog.F.t_a[i]; r[HO::t_b + i] = prog.F.t_b[i]; }
#pragma unroll
            for (int c = 0; c < MAXC; ++c) if (c < P.ncontact) for (int i = 0; i < 18; ++i) r[HO::G134 + HO::per_G134 * c + i] = prog.ccold(c).G134[i];
        }
        r[HO::flag] = (RF || status == DJ_STATUS_DEFERRED) ? T(1) : T(0);
    }
    if (!RF && A.flag && active && q == 0 && k == 0) A.flag[env] = status == DJ_STATUS_DEFERRED ? 1 : 0;
    if (QUAD && A.fac && (!RF || active)) {
        T* f = A.fac + (size_t)wave_index * FAC_PER_LANE * wv.width() + lane;
        const int W = wv.width();
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 12; ++j) f[(size_t)(FAC_S + 12 * i + j) * W] = T(prog.F.Sq[i][j]);
#pragma unroll
            for (int j = 0; j < 6; ++j) { f[(size_t)(FAC_U + 6 * i + j) * W] = T(prog.F.Uq[i][j]); f[(size_t)(FAC_L + 6 * i + j) * W] = T(prog.F.Lq[j][i]); }
        }
    }
    if (active && q == 0) {
        T zn[13];
        prog.next_state(zn);
        TIO* o = A.z_next + (size_t)env * 13 * G.Nb + 13 * k;
        for (int i = 0; i < 13; ++i) o[i] = TIO(zn[i]);
        if (k == 0) { if (A.status) A.status[env] = status; if (A.iters) A.iters[env] = iters; if (A.mu_out) A.mu_out[env] = prog.mu; }
        if constexpr (QUAD && DJ_REFINE) { if (k == 0 && A.diag_out) { A.diag_out[2 * env] = prog.wstiff; A.diag_out[2 * env + 1] = gr_env; } }
        if (A.vel) { TIO* vo = A.vel + (size_t)env * 6 * G.Nb + 6 * k; for (int i = 0; i < 3; ++i) { vo[i] = TIO(prog.L.v[i]); vo[3 + i] = TIO(prog.L.w[i]); } }
        if (A.res) { TIO* ro = A.res + (size_t)env * 6 * G.Nb + 6 * k; for (int i = 0; i < 6; ++i) ro[i] = TIO(prog.rb[i]); }
#ifdef DJ_PROF2
        if (A.vel && k == 4 && G.Nb >= 9) { TIO* vo = A.vel + (size_t)env * 6 * G.Nb + 24; for (int i = 0; i < 24; ++i) vo[i] = TIO((double)prog.p2c[i]); }
#endif
#ifdef DJ_PROF
        if (A.vel && k == 0) { TIO* vo = A.vel + (size_t)env * 6 * G.Nb; for (int i = 0; i < 6; ++i) vo[i] = TIO((double)prog.pc[i]); }   // phases 0-5 (cycles)
        if (A.vel && k == 1) { TIO* vo = A.vel + (size_t)env * 6 * G.Nb + 6; vo[0] = TIO((double)prog.pc[7]); vo[1] = TIO((double)iters); vo[2] = TIO((double)prog.pc[6]); }
#endif
        if (A.joint_imp && P.n_imp > 0) {
            // get_solution order per joint: [tra: λ_t] [rot: s_up s_lo γ_up γ_lo λ_r]   (translational limits unsupported)
            TIO* jo = A.joint_imp + (size_t)env * G.n_joint_imp + P.imp_off;
            int o2 = 0;
            if (prog.tlim) { jo[o2++] = TIO(prog.L.ls[0]); jo[o2++] = TIO(prog.L.ls[1]); jo[o2++] = TIO(prog.L.lg[0]); jo[o2++] = TIO(prog.L.lg[1]); }   // [tra: s_up s_lo γ_up γ_lo λ_t]
#if DJ_MLIM
            // limits on several coordinates: η = [s_up(n); s_lo(n); γ_up(n); γ_lo(n); λ] per half (split_impulses, src/joints/joint.jl)
            if (prog.kMLim && prog.nlm() > 0) { const int nt_ = prog.mlp->nt;
                for (int i = 0; i < 2; ++i) for (int m = 0; m < nt_; ++m) jo[o2++] = TIO(prog.L.mls[m][i]);
                for (int i = 0; i < 2; ++i) for (int m = 0; m < nt_; ++m) jo[o2++] = TIO(prog.L.mlg[m][i]); }
#endif
            for (int i = 0; i < 3; ++i) if (i < P.nl_t) jo[o2++] = TIO(prog.L.lam[i]);
            if (P.nlim_r > 0) { jo[o2++] = TIO(prog.L.ls[0]); jo[o2++] = TIO(prog.L.ls[1]); jo[o2++] = TIO(prog.L.lg[0]); jo[o2++] = TIO(prog.L.lg[1]); }
#if DJ_MLIM
            if (prog.kMLim && prog.nlm() > 0) { const int nt_ = prog.mlp->nt, nr_ = prog.mlp->nr;
                for (int i = 0; i < 2; ++i) for (int m = 0; m < nr_; ++m) jo[o2++] = TIO(prog.L.mls[nt_ + m][i]);
                for (int i = 0; i < 2; ++i) for (int m = 0; m < nr_; ++m) jo[o2++] = TIO(prog.L.mlg[nt_ + m][i]); }
#endif
            for (int i = 0; i < 3; ++i) if (i < P.nl_r) jo[o2++] = TIO(prog.L.lam[3 + i]);
        }
#if DJ_CUT
        if constexpr (!QUAD) { if (A.joint_imp && k == 0) for (int c = 0; c < NCUT; ++c) if (c < prog.ncut) {     // the cut joints' multipliers, get_solution order [λ_t; λ_r]
            TIO* jo = A.joint_imp + (size_t)env * G.n_joint_imp + A.cuts[c].imp_off; int o2 = 0;
            for (int i = 0; i < 3; ++i) if (i < A.cuts[c].nl_t) jo[o2++] = TIO(prog.clam[c][i]);
            for (int i = 0; i < 3; ++i) if (i < A.cuts[c].nl_r) jo[o2++] = TIO(prog.clam[c][3 + i]);
        } }
#endif
        if (A.contact_sg) {
#pragma unroll
            for (int c = 0; c < MAXC; ++c) if (c < P.ncontact) {
                TIO* co = A.contact_sg + (size_t)env * (2 * NCV) * G.Nc + (2 * NCV) * P.contact[c];       // [s; γ] per contact (8; LinearContact builds: 12)
                for (int i = 0; i < NCV; ++i) { co[i] = TIO(prog.L.cs[c][i]); co[NCV + i] = TIO(prog.L.cg[c][i]); }
            }
        }
    }
}

} // namespace dj
