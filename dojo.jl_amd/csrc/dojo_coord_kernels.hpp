// dojo_coord_kernels.hpp -- the kernels around the step that work on coordinates: minimal <-> maximal coordinates, their
// Jacobians and the chain of get_minimal_gradients!, the contact part of an observation, the Storage rows, get_next_state and the impulse fold
// of dojo_step_impulses.  HBM-bound helper kernels; every DojoEnvironments step! goes through the two maps (src/simulation/step.jl:42-60).
// The per-joint maps live in dojo_coords.hpp, written for any scalar: double gives the values, forward-mode dual numbers give the chain-rule
// Jacobians of get_minimal_gradients! (src/gradients/state.jl:9-56, 136-217).
// x per joint (mechanism.joints order): [dx(nu_t); dtheta(nu_r); dv(nu_t); domega(nu_r)]
//
// The kernels take raw pointers and the tables.  Their grids, casts and the handle's buffers are dojo_hip.hip's: one launch_*<TIO> per kernel.
#pragma once
#include <hip/hip_runtime.h>
#include "dojo_coords.hpp"

namespace dj {
namespace ckern {
using namespace dj::coords;
// (load_body, origin_body: dojo_coords.hpp -- the policy kernel of dojo_policy.hpp reads bodies the same way)
// get_next_state (src/mechanism/get.jl:126-134) of a body whose velocities are its solution: x + dt v, q (x) xi(w)
template <class S> __device__ __forceinline__ void advance_body(PoseVel<S>& p, double dt) {
    for (int i = 0; i < 3; ++i) p.x[i] = p.x[i] + p.v[i] * dt;
    S qn[4]; next_qS(qn, p.q, p.w, dt); for (int i = 0; i < 4; ++i) p.q[i] = qn[i];
}

// one thread per environment: bodies in root -> leaves order (the parent's maximal state must exist first)
template <class TIO>
__global__ void min2max_kernel(const NodeP<double>* nodes, const int* order, int Nb, int nu, double dt, int B, const TIO* x, TIO* z) {
    const int env = blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= B) return;
    const TIO* xe = x + (size_t)env * 2 * nu; TIO* ze = z + (size_t)env * 13 * Nb;
    for (int oi = 0; oi < Nb; ++oi) {
        const int k = order[oi];
        const NodeP<double>& P = nodes[k];
        const int nt = P.nu_t, nr = P.nu_r, n = nt + nr;
        const TIO* xm = xe + 2 * P.u_off;
        double dx[3] = {0, 0, 0}, dth[3] = {0, 0, 0}, dv[3] = {0, 0, 0}, dw[3] = {0, 0, 0};
        for (int i = 0; i < 3; ++i) { if (i < nt) { dx[i] = (double)xm[i]; dv[i] = (double)xm[n + i]; } if (i < nr) { dth[i] = (double)xm[nt + i]; dw[i] = (double)xm[n + nt + i]; } }
        const PoseVel<double> a = P.parent >= 0 ? load_body<double>(ze, P.parent) : origin_body<double>();
        PoseVel<double> b;
        joint_min2max(b, P, dt, a, dx, dth, dv, dw);
        for (int i = 0; i < 3; ++i) { ze[13 * k + i] = (TIO)b.x[i]; ze[13 * k + 3 + i] = (TIO)b.v[i]; ze[13 * k + 10 + i] = (TIO)b.w[i]; }
        for (int i = 0; i < 4; ++i) ze[13 * k + 6 + i] = (TIO)b.q[i];
    }
}
// one thread per (environment, joint): the joints are independent
template <class TIO>
__global__ void max2min_kernel(const NodeP<double>* nodes, int Nb, int nu, double dt, int B, const TIO* z, TIO* x, int ldx) {
    const int tid = blockIdx.x * blockDim.x + threadIdx.x;
    const int env = tid / Nb, k = tid % Nb;
    if (env >= B) return;
    const NodeP<double>& P = nodes[k];
    const TIO* ze = z + (size_t)env * 13 * Nb; TIO* xm = x + (size_t)env * ldx + 2 * P.u_off;
    const int nt = P.nu_t, nr = P.nu_r, n = nt + nr;
    const PoseVel<double> b = load_body<double>(ze, k), a = P.parent >= 0 ? load_body<double>(ze, P.parent) : origin_body<double>();
    double ct[3], cr[3], vt[3], vr[3];
    joint_max2min(ct, cr, vt, vr, P, dt, a, b);
    for (int i = 0; i < 3; ++i) { if (i < nt) { xm[i] = (TIO)ct[i]; xm[n + i] = (TIO)vt[i]; } if (i < nr) { xm[nt + i] = (TIO)cr[i]; xm[n + nt + i] = (TIO)vr[i]; } }
}

// the contact part of get_state(::AntARS) (DojoEnvironments/src/environments/ant_ars.jl:72-80): the normal impulse of
// every contact, clamped to [-1, 1], behind the minimal state.  csg = [s(4); gamma(4)] per contact of the last step.
template <class TIO>
__global__ void contact_obs_kernel(int Nc, int B, const TIO* csg, TIO* obs, int ldx, int off) {
    const int tid = blockIdx.x * blockDim.x + threadIdx.x;
    const int env = tid / Nc, c = tid % Nc;
    if (env >= B) return;
    const double g = (double)csg[(size_t)env * 8 * Nc + 8 * c + 4];
    obs[(size_t)env * ldx + off + c] = (TIO)(g < -1.0 ? -1.0 : g > 1.0 ? 1.0 : g);
}

// save_to_storage! (src/simulation/storage.jl:50-67): one thread per (environment, body); inputs are the state the step
// was solved at and what the step kernel left behind (solution velocities, cone variables, body residual rows)
template <class TIO>
__global__ void storage_kernel(const NodeP<double>* nodes, const ContactP<double>* contacts, int Nb, int Nc, int model, int cper, double dt, int env0, int nenv,
                               const TIO* z, const TIO* vel, const TIO* csg, const TIO* res, const TIO* fext, TIO* storage) {
    const int tid = blockIdx.x * blockDim.x + threadIdx.x;
    const int e = tid / Nb, k = tid % Nb;
    if (e >= nenv) return;
    const size_t env = (size_t)env0 + e;
    double zb[13], v[3], w[3], rb[6], row[25], fe[6];
    if (fext) for (int i = 0; i < 6; ++i) fe[i] = (double)fext[env * 6 * Nb + 6 * k + i];
    for (int i = 0; i < 13; ++i) zb[i] = (double)z[env * 13 * Nb + 13 * k + i];
    for (int i = 0; i < 3; ++i) { v[i] = (double)vel[env * 6 * Nb + 6 * k + i]; w[i] = (double)vel[env * 6 * Nb + 6 * k + 3 + i]; }
    for (int i = 0; i < 6; ++i) rb[i] = (double)res[env * 6 * Nb + 6 * k + i];
    auto other = [=](int b, double* zo, double* vo, double* wo) {            // (body-body contacts: the contact partner's state and solution)
        for (int i = 0; i < 13; ++i) zo[i] = (double)z[env * 13 * Nb + 13 * b + i];
        for (int i = 0; i < 3; ++i) { vo[i] = (double)vel[env * 6 * Nb + 6 * b + i]; wo[i] = (double)vel[env * 6 * Nb + 6 * b + 3 + i]; }
    };
    dj::storage_row(row, nodes[k], contacts, dt, zb, v, w, csg + env * (size_t)cper * Nc, rb, fext ? fe : (const double*)nullptr, nodes, other, model, cper, k, Nc);
    TIO* o = storage + (env * Nb + k) * 25;
    for (int i = 0; i < 25; ++i) o[i] = (TIO)row[i];
}

// ---- Jacobians by forward-mode differentiation of the same maps ----
typedef Dual<24> D24;
// minimal_to_maximal_jacobian (src/gradients/state.jl:136-181): one thread per environment, root -> leaves;
// Jm[env][12 Nb rows][2 nu columns] row-major.  z must already hold minimal_to_maximal(x).
template <class TIO>
__global__ void min2max_jac_kernel(const NodeP<double>* nodes, const int* order, int Nb, int nu, double dt, int B, const TIO* x, const TIO* z, double* Jm) {
    const int env = blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= B) return;
    const int nm = 2 * nu;
    const TIO* xe = x + (size_t)env * nm; const TIO* ze = z + (size_t)env * 13 * Nb;
    double* J = Jm + (size_t)env * 12 * Nb * nm;
    for (int oi = 0; oi < Nb; ++oi) {
        const int k = order[oi];
        const NodeP<double>& P = nodes[k];
        const int nt = P.nu_t, nr = P.nu_r, n = nt + nr;
        const TIO* xm = xe + 2 * P.u_off;
        // directions 0..11: the parent's reduced state; 12..12+2n-1: the joint's own minimal coordinates in layout order
        D24 dx[3], dth[3], dv[3], dw[3];
        for (int i = 0; i < 3; ++i) {
            dx[i] = i < nt ? D24::seed((double)xm[i], 12 + i) : D24(0.0);             dv[i] = i < nt ? D24::seed((double)xm[n + i], 12 + n + i) : D24(0.0);
            dth[i] = i < nr ? D24::seed((double)xm[nt + i], 12 + nt + i) : D24(0.0);    dw[i] = i < nr ? D24::seed((double)xm[n + nt + i], 12 + n + nt + i) : D24(0.0);
        }
        const PoseVel<double> a0 = P.parent >= 0 ? load_body<double>(ze, P.parent) : origin_body<double>();
        PoseVel<D24> a = seed_body<24>(a0, 0), b;
        joint_min2max(b, P, dt, a, dx, dth, dv, dw);
        // rows of the child: x, v, phi = V(q_b^-1 (x) dq_b), omega
        double Pm[12][24];
        for (int d = 0; d < 24; ++d) {
            for (int i = 0; i < 3; ++i) { Pm[i][d] = b.x[i].d[d]; Pm[3 + i][d] = b.v[i].d[d]; Pm[9 + i][d] = b.w[i].d[d]; }
            const double q0 = b.q[0].v, q1 = b.q[1].v, q2 = b.q[2].v, q3 = b.q[3].v, e0 = b.q[0].d[d], e1 = b.q[1].d[d], e2 = b.q[2].d[d], e3 = b.q[3].d[d];
            Pm[6][d] = q0 * e1 - q1 * e0 - q2 * e3 + q3 * e2;                 // vector part of conj(q) (x) dq
            Pm[7][d] = q0 * e2 + q1 * e3 - q2 * e0 - q3 * e1;
            Pm[8][d] = q0 * e3 - q1 * e2 + q2 * e1 - q3 * e0;
        }
        for (int r = 0; r < 12; ++r) {
            double* Jr = J + (size_t)(12 * k + r) * nm;
            for (int c = 0; c < nm; ++c) {
                double acc = 0.0;
                if (P.parent >= 0) { const double* Jp = J + (size_t)(12 * P.parent) * nm + c; for (int m = 0; m < 12; ++m) acc += Pm[r][m] * Jp[(size_t)m * nm]; }
                const int lc = c - 2 * P.u_off;
                if (lc >= 0 && lc < 2 * n) acc += Pm[r][12 + lc];
                Jr[c] = acc;
            }
        }
    }
}
// maximal_to_minimal_jacobian (src/gradients/state.jl:9-56) at z (advanced by one integrator step when `advance`):
// one thread per (environment, joint); Jb[env][joint k][2n rows in layout order][24]: d/d(parent reduced state), d/d(child)
template <class TIO>
__global__ void max2min_jac_kernel(const NodeP<double>* nodes, int Nb, double dt, int B, const TIO* z, int advance, double* Jb) {
    const int tid = blockIdx.x * blockDim.x + threadIdx.x;
    const int env = tid / Nb, k = tid % Nb;
    if (env >= B) return;
    const NodeP<double>& P = nodes[k];
    const TIO* ze = z + (size_t)env * 13 * Nb;
    const int nt = P.nu_t, nr = P.nu_r, n = nt + nr;
    PoseVel<double> b0 = load_body<double>(ze, k), a0 = P.parent >= 0 ? load_body<double>(ze, P.parent) : origin_body<double>();
    if (advance) { advance_body(b0, dt); if (P.parent >= 0) advance_body(a0, dt); }
    PoseVel<D24> a = seed_body<24>(a0, 0), b = seed_body<24>(b0, 12);
    D24 ct[3], cr[3], vt[3], vr[3];
    joint_max2min(ct, cr, vt, vr, P, dt, a, b);
    double* o = Jb + ((size_t)env * Nb + k) * 12 * 24;
    for (int i = 0; i < 3; ++i) for (int d = 0; d < 24; ++d) {
        if (i < nt) { o[(size_t)i * 24 + d] = ct[i].d[d]; o[(size_t)(n + i) * 24 + d] = vt[i].d[d]; }
        if (i < nr) { o[(size_t)(nt + i) * 24 + d] = cr[i].d[d]; o[(size_t)(n + nt + i) * 24 + d] = vr[i].d[d]; }
    }
}
// T = dz * Jm  (12Nb x 2nu per environment); dz is column-major per environment: dz(r, c) = dz[c * nx + r]
template <class TIO>
__global__ void chain_mid_kernel(int nx, int nm, int B, const TIO* dz, const double* Jm, double* T) {
    const int env = blockIdx.x;
    const TIO* D = dz + (size_t)env * nx * nx; const double* J = Jm + (size_t)env * nx * nm; double* Te = T + (size_t)env * nx * nm;
    for (int e = threadIdx.x; e < nx * nm; e += blockDim.x) {
        const int r = e % nx, j = e / nx;                                       // consecutive threads -> consecutive rows (coalesced dz reads)
        double acc = 0.0;
        for (int c = 0; c < nx; ++c) acc += (double)D[(size_t)c * nx + r] * J[(size_t)c * nm + j];
        Te[(size_t)r * nm + j] = acc;
    }
}
// jx = M2m * T, ju = M2m * du with the block-sparse M2m (each joint's rows touch its parent's and its child's 12 columns);
// outputs row-major per environment: jx[env][2nu][2nu], ju[env][2nu][nu]; du(r, c) = du[c * nx + r]
template <class TIO>
__global__ void chain_out_kernel(const NodeP<double>* nodes, int Nb, int nu, int B, const double* Jb, const double* T, const TIO* du, TIO* jx, TIO* ju) {
    const int env = blockIdx.x, nx = 12 * Nb, nm = 2 * nu;
    const double* Te = T + (size_t)env * nx * nm; const TIO* Du = du ? du + (size_t)env * nx * nu : nullptr;
    for (int e = threadIdx.x; e < nm * (nm + nu); e += blockDim.x) {
        const int i = e / (nm + nu), j = e % (nm + nu);
        // joint owning minimal row i
        int k = 0, lr = 0;
        for (int b = 0; b < Nb; ++b) { const int o = 2 * nodes[b].u_off, nn = 2 * (nodes[b].nu_t + nodes[b].nu_r); if (i >= o && i < o + nn) { k = b; lr = i - o; } }
        const double* Jr = Jb + (((size_t)env * Nb + k) * 12 + lr) * 24;
        const int par = nodes[k].parent;
        double acc = 0.0;
        for (int m = 0; m < 12; ++m) {
            if (j < nm) { if (par >= 0) acc += Jr[m] * Te[(size_t)(12 * par + m) * nm + j]; acc += Jr[12 + m] * Te[(size_t)(12 * k + m) * nm + j]; }
            else if (Du) { const int c = j - nm; if (par >= 0) acc += Jr[m] * (double)Du[(size_t)c * nx + 12 * par + m]; acc += Jr[12 + m] * (double)Du[(size_t)c * nx + 12 * k + m]; }
        }
        if (j < nm) jx[((size_t)env * nm + i) * nm + j] = (TIO)acc; else if (ju) ju[((size_t)env * nm + i) * nu + (j - nm)] = (TIO)acc;
    }
}
// get_next_state(mechanism) (src/mechanism/get.jl:126-134) of bodies whose stored velocities are their solution: one thread per (env, body)
template <class TIO>
__global__ void next_state_kernel(int Nb, double dt, int B, const TIO* z, TIO* zo) {
    const int tid = blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= B * Nb) return;
    PoseVel<double> p = load_body<double>(z + (size_t)(tid / Nb) * 13 * Nb, tid % Nb);
    advance_body(p, dt);
    TIO* o = zo + (size_t)tid * 13;
    for (int i = 0; i < 3; ++i) { o[i] = (TIO)p.x[i]; o[3 + i] = (TIO)p.v[i]; o[10 + i] = (TIO)p.w[i]; }
    for (int i = 0; i < 4; ++i) o[6 + i] = (TIO)p.q[i];
}
// dojo_step_impulses: external force + body impulses / dt
template <class TIO> __global__ void fold_impulses_kernel(long long n, const TIO* fext, const TIO* jf, double inv_dt, TIO* out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (TIO)((fext ? (double)fext[i] : 0.0) + (double)jf[i] * inv_dt);
}

} // namespace ckern
} // namespace dj
