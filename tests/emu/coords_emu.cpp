// coords_emu.cpp -- the per-joint coordinate templates of dojo.jl_amd/csrc/dojo_coords.hpp on the host (TEST INFRASTRUCTURE).
//
// The coordinate kernels of dojo_coord_kernels.hpp are thin wrappers around coords::joint_min2max / coords::joint_max2min, instantiated for double (the maps)
// and Dual<24> (their Jacobians).  This file instantiates the same templates with g++ for ONE environment, so the CPU tier can pin the series
// branches and the dual arithmetic against the oracle (tests/test_coords_emu.py); what is left to the GPU tier is the kernels' indexing and launches.
// The loops below restate min2max_kernel, max2min_kernel, min2max_jac_kernel and max2min_jac_kernel for fp64 buffers.  Not a product path.
#include "../../dojo.jl_amd/csrc/dojo_host.hpp"
#include "../../dojo.jl_amd/csrc/dojo_coords.hpp"

namespace {
using namespace dj;
using namespace dj::coords;
typedef Dual<24> D24;

// bodies root -> leaves, as the handle orders them (dojo_hip.hip: d_order)
std::vector<int> order_of(const HostModel& M) {
    std::vector<int> order;
    for (int lev = 0; lev <= M.maxlevel; ++lev) for (int b = 0; b < M.Nb; ++b) if (M.nodes[b].level == lev) order.push_back(b);
    return order;
}
int model_of(const DojoTopology* tp, HostModel& M) {
    const int rc = build_host_model(*tp, M);
    if (rc != DOJO_OK) return rc;
    return M.has_loop ? DOJO_ERR_UNSUPPORTED : DOJO_OK;
}
}

extern "C" {

// z [13 Nb] = minimal_to_maximal(x [2 nu])
int coords_min2max(const DojoTopology* tp, const double* x, double* z) {
    HostModel M; int rc = model_of(tp, M); if (rc) return rc;
    for (int k : order_of(M)) {
        const NodeP<double>& P = M.nodes[k];
        const int nt = P.nu_t, nr = P.nu_r, n = nt + nr;
        const double* xm = x + 2 * P.u_off;
        double dx[3] = {0, 0, 0}, dth[3] = {0, 0, 0}, dv[3] = {0, 0, 0}, dw[3] = {0, 0, 0};
        for (int i = 0; i < 3; ++i) { if (i < nt) { dx[i] = xm[i]; dv[i] = xm[n + i]; } if (i < nr) { dth[i] = xm[nt + i]; dw[i] = xm[n + nt + i]; } }
        const PoseVel<double> a = P.parent >= 0 ? load_body<double>(z, P.parent) : origin_body<double>();
        PoseVel<double> b;
        joint_min2max(b, P, M.dt, a, dx, dth, dv, dw);
        for (int i = 0; i < 3; ++i) { z[13 * k + i] = b.x[i]; z[13 * k + 3 + i] = b.v[i]; z[13 * k + 10 + i] = b.w[i]; }
        for (int i = 0; i < 4; ++i) z[13 * k + 6 + i] = b.q[i];
    }
    return DOJO_OK;
}

// x [2 nu] = maximal_to_minimal(z [13 Nb])
int coords_max2min(const DojoTopology* tp, const double* z, double* x) {
    HostModel M; int rc = model_of(tp, M); if (rc) return rc;
    for (int k = 0; k < M.Nb; ++k) {
        const NodeP<double>& P = M.nodes[k];
        const int nt = P.nu_t, nr = P.nu_r, n = nt + nr;
        double* xm = x + 2 * P.u_off;
        const PoseVel<double> b = load_body<double>(z, k), a = P.parent >= 0 ? load_body<double>(z, P.parent) : origin_body<double>();
        double ct[3], cr[3], vt[3], vr[3];
        joint_max2min(ct, cr, vt, vr, P, M.dt, a, b);
        for (int i = 0; i < 3; ++i) { if (i < nt) { xm[i] = ct[i]; xm[n + i] = vt[i]; } if (i < nr) { xm[nt + i] = cr[i]; xm[n + nt + i] = vr[i]; } }
    }
    return DOJO_OK;
}

// Jm [12 Nb][2 nu] row-major = minimal_to_maximal_jacobian(x); z must hold minimal_to_maximal(x)
int coords_min2max_jacobian(const DojoTopology* tp, const double* x, const double* z, double* Jm) {
    HostModel M; int rc = model_of(tp, M); if (rc) return rc;
    const int nm = 2 * M.nu;
    for (int k : order_of(M)) {
        const NodeP<double>& P = M.nodes[k];
        const int nt = P.nu_t, nr = P.nu_r, n = nt + nr;
        const double* xm = x + 2 * P.u_off;
        D24 dx[3], dth[3], dv[3], dw[3];
        for (int i = 0; i < 3; ++i) {
            dx[i] = i < nt ? D24::seed(xm[i], 12 + i) : D24(0.0);             dv[i] = i < nt ? D24::seed(xm[n + i], 12 + n + i) : D24(0.0);
            dth[i] = i < nr ? D24::seed(xm[nt + i], 12 + nt + i) : D24(0.0);    dw[i] = i < nr ? D24::seed(xm[n + nt + i], 12 + n + nt + i) : D24(0.0);
        }
        const PoseVel<double> a0 = P.parent >= 0 ? load_body<double>(z, P.parent) : origin_body<double>();
        PoseVel<D24> a = seed_body<24>(a0, 0), b;
        joint_min2max(b, P, M.dt, a, dx, dth, dv, dw);
        double Pm[12][24];
        for (int d = 0; d < 24; ++d) {
            for (int i = 0; i < 3; ++i) { Pm[i][d] = b.x[i].d[d]; Pm[3 + i][d] = b.v[i].d[d]; Pm[9 + i][d] = b.w[i].d[d]; }
            const double q0 = b.q[0].v, q1 = b.q[1].v, q2 = b.q[2].v, q3 = b.q[3].v, e0 = b.q[0].d[d], e1 = b.q[1].d[d], e2 = b.q[2].d[d], e3 = b.q[3].d[d];
            Pm[6][d] = q0 * e1 - q1 * e0 - q2 * e3 + q3 * e2;                 // vector part of conj(q) (x) dq
            Pm[7][d] = q0 * e2 + q1 * e3 - q2 * e0 - q3 * e1;
            Pm[8][d] = q0 * e3 - q1 * e2 + q2 * e1 - q3 * e0;
        }
        for (int r = 0; r < 12; ++r) for (int c = 0; c < nm; ++c) {
            double acc = 0.0;
            if (P.parent >= 0) for (int m = 0; m < 12; ++m) acc += Pm[r][m] * Jm[(size_t)(12 * P.parent + m) * nm + c];
            const int lc = c - 2 * P.u_off;
            if (lc >= 0 && lc < 2 * n) acc += Pm[r][12 + lc];
            Jm[(size_t)(12 * k + r) * nm + c] = acc;
        }
    }
    return DOJO_OK;
}

// JM [2 nu][12 Nb] row-major (dense) = maximal_to_minimal_jacobian(z)
int coords_max2min_jacobian(const DojoTopology* tp, const double* z, double* JM) {
    HostModel M; int rc = model_of(tp, M); if (rc) return rc;
    const int nx = 12 * M.Nb;
    for (int i = 0; i < 2 * M.nu * nx; ++i) JM[i] = 0.0;
    for (int k = 0; k < M.Nb; ++k) {
        const NodeP<double>& P = M.nodes[k];
        const int nt = P.nu_t, nr = P.nu_r, n = nt + nr;
        const PoseVel<double> b0 = load_body<double>(z, k), a0 = P.parent >= 0 ? load_body<double>(z, P.parent) : origin_body<double>();
        const PoseVel<D24> a = seed_body<24>(a0, 0), b = seed_body<24>(b0, 12);
        D24 ct[3], cr[3], vt[3], vr[3];
        joint_max2min(ct, cr, vt, vr, P, M.dt, a, b);
        auto put = [&](int row, const D24& v) {
            double* o = JM + (size_t)(2 * P.u_off + row) * nx;
            for (int d = 0; d < 12; ++d) { if (P.parent >= 0) o[12 * P.parent + d] = v.d[d]; o[12 * k + d] = v.d[12 + d]; }
        };
        for (int i = 0; i < 3; ++i) { if (i < nt) { put(i, ct[i]); put(n + i, vt[i]); } if (i < nr) { put(nt + i, cr[i]); put(n + nt + i, vr[i]); } }
    }
    return DOJO_OK;
}

}
