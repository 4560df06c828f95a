"""Rollouts as a differentiable torch operation (torch is plumbing only: it owns the buffers and the graph; the rollout, the IFT
Jacobians and the reverse sweep are the library's kernels, include/dojo_hip.h "Reverse-mode rollouts").

    Z = differentiable_rollout(mech, z0, U)          # z0 [B,13Nb], U [H,B,nu] device tensors -> Z [H,B,13Nb]
    loss(Z).backward()                               # U.grad [H,B,nu], z0.grad [B,13Nb]

    Z, OBS, U = differentiable_policy_rollout(mech, z0, W, bias=b, U_ff=Uff)     # closed loop: u_k = U_ff[k] + E (b + W ((o_k - mean) .* scale))
    loss(Z, OBS, U).backward()                       # W.grad, b.grad, Uff.grad, z0.grad

    theta = torch.cat([t.reshape(-1) for layer in net for t in (layer.weight, layer.bias)])      # a torch.nn tanh MLP in the layout of api.pack_mlp
    Z, OBS, U = differentiable_mlp_rollout(mech, z0, theta, widths, U_ff=Uff)      # closed loop through the network
    loss(Z, OBS, U).backward()                       # reaches the modules' parameters through the cat

    Z = differentiable_data_rollout(mech, z0, U, theta)      # theta [Nc,5] fp64: the contact data (system identification)
    loss(Z).backward()                               # theta.grad [Nc,5], U.grad, z0.grad

Everything is enqueued on torch's current stream and nothing synchronizes.  The gradient is the chain of the handle's gradient mode:
set `mech.set_gradient_mode(api.GRAD_CONSISTENT)` for the derivative of the rollout.
"""
import ctypes as C

import torch

from . import api


def lift_tangent(gz, z0):
    """[B,nx] tangent cotangent -> [B,13Nb] state cotangent at z0: g_x, g_v, g_omega are copied and g_q = q0 (x) (0, g_phi), the transpose's
    right inverse on the tangent space of the unit sphere at q0 (a 4-byte z0 stands for q0 / |q0|, as in the kernels)."""
    B = z0.shape[0]
    g = gz.double().reshape(B, -1, 12); z = z0.double().reshape(B, -1, 13)
    q = z[..., 6:10]; q = q / q.norm(dim=-1, keepdim=True) if z0.dtype == torch.float32 else q
    s, v, p = q[..., :1], q[..., 1:], g[..., 6:9]
    gq = torch.cat([-(v * p).sum(-1, keepdim=True), s * p + torch.linalg.cross(v, p)], -1)
    return torch.cat([g[..., 0:6], gq, g[..., 9:12]], -1).reshape(B, -1).to(z0.dtype)


def _dtype(mech):
    return torch.float32 if mech.dtype_code == 1 else torch.float64


def _want(t, what, dt, shapes, shown=None):
    """None, or the device tensor t of dtype dt and one of `shapes`, contiguous (shown: how the message writes the shape)"""
    if t is None:
        return None
    if not t.is_cuda or t.dtype != dt or tuple(t.shape) not in shapes:
        raise ValueError("%s must be a %s device tensor of shape %s" % (what, dt, shown or " or ".join(str(x) for x in shapes)))
    return t.contiguous()


def _horizon(U, what, steps, dt, B, nu, shown=None):
    """-> (H, U contiguous): the horizon is the leading dimension of the controls [H,B,nu], or `steps` without them"""
    if U is None:
        return int(steps), None
    H = int(U.shape[0]) if U.dim() else 0
    return H, _want(U, what, dt, [(H, B, nu)], shown)


def _controls(mech, U, steps):
    """-> (H, U contiguous) of an open-loop rollout (a mechanism without inputs takes no controls)"""
    s, B = mech.spec, mech.batch
    return _horizon(U if s.nu else None, "U", steps, _dtype(mech), B, s.nu, "(H, %d, %d)" % (B, s.nu))


def _record(mech, H, dev, closed_loop=False):
    """-> Z, status, DZ, DU (and OBS, U of a closed loop): the tensors a recording rollout writes; the Jacobians are freed with the graph"""
    s, B, dt = mech.spec, mech.batch, _dtype(mech)
    Z = torch.empty((H, B, s.nz), dtype=dt, device=dev)
    status = torch.empty((H, B), dtype=torch.int32, device=dev)
    DZ = torch.empty((H, B, s.nx, s.nx), dtype=dt, device=dev)
    DU = torch.empty((H, B, s.nu, s.nx), dtype=dt, device=dev) if (s.nu or closed_loop) else None
    if not closed_loop:
        return Z, status, DZ, DU
    return Z, status, DZ, DU, torch.empty((H + 1, B, 2 * s.nu), dtype=dt, device=dev), torch.empty((H, B, s.nu), dtype=dt, device=dev)


def _cotangents(Z, gZ, *optional):
    """the incoming cotangents, contiguous; one torch leaves out is a zero: the state's is required by the ABI, the others are optional (None)"""
    return (torch.zeros_like(Z) if gZ is None else gZ.contiguous(),) + tuple(None if g is None else g.contiguous() for g in optional)


class _Rollout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mech, z0, U, steps):
        z0c = _want(z0, "z0", _dtype(mech), [(mech.batch, mech.spec.nz)])
        H, Uc = _controls(mech, U, steps)
        dev = z0.device
        Z, status, DZ, DU = _record(mech, H, dev)
        api._chk(api.lib().dojo_rollout_record_dev(mech.h, api.addr(z0c), api.addr(Uc), H, api.addr(Z), api.addr(status), api.addr(DZ), api.addr(DU), api.torch_stream(dev)))
        ctx.mech, ctx.H, ctx.has_u = mech, H, U is not None
        ctx.save_for_backward(z0c, Z, status, DZ, *([DU] if DU is not None else []))
        ctx.mark_non_differentiable(status)
        return Z, status

    @staticmethod
    def backward(ctx, gZ, _gstatus):
        mech, H = ctx.mech, ctx.H
        s, B = mech.spec, mech.batch
        z0, Z, status, DZ = ctx.saved_tensors[:4]
        DU = ctx.saved_tensors[4] if len(ctx.saved_tensors) > 4 else None
        gZ, = _cotangents(Z, gZ)
        want_u = ctx.has_u and s.nu > 0 and ctx.needs_input_grad[2]
        gU = torch.empty((H, B, s.nu), dtype=Z.dtype, device=Z.device) if want_u else None
        gz = torch.empty((B, s.nx), dtype=Z.dtype, device=Z.device) if ctx.needs_input_grad[1] else None
        api._chk(api.lib().dojo_rollout_adjoint_dev(mech.h, H, api.addr(DZ), api.addr(DU), api.addr(gZ), 1, api.addr(Z), api.addr(status), api.addr(gU), api.addr(gz), api.torch_stream(Z.device)))
        return None, (lift_tangent(gz, z0) if gz is not None else None), gU, None


def differentiable_rollout(mech, z0, U=None, steps=None):
    """-> Z [H,B,13Nb], the states after every step of the rollout from z0 under the controls U [H,B,nu] (None with `steps`: no controls), as a
    node of torch's graph.  Forward: dojo_rollout_record_dev into torch-owned tensors (the Jacobians of every step, H B nx (nx + nu) scalars, live
    as long as the graph); backward: one dojo_rollout_adjoint_dev launch with the state-space cotangent of Z.

    The gradient w.r.t. z0 is the tangent-space gradient lifted to state shape per body: g_q = q0 (x) (0, g_phi), i.e. the gradient restricted to
    the unit sphere of quaternions (its component along q0, which no rollout can see, is zero); x, v, omega are plain.  Nothing flows through a
    failed step.  Z.status [H,B] (int32, non-differentiable) is the solver status of every step."""
    Z, status = _Rollout.apply(mech, z0, U, steps)
    Z.status = status
    return Z


class _DataRollout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mech, z0, U, theta, steps):
        s, B, dt = mech.spec, mech.batch, _dtype(mech)
        Nc = len(s.contacts)
        z0c = _want(z0, "z0", dt, [(B, s.nz)])
        if theta is None or theta.dtype != torch.float64 or tuple(theta.shape) != (Nc, 5):
            raise ValueError("theta must be a float64 tensor of shape %s" % ((Nc, 5),))
        H, Uc = _controls(mech, U, steps)
        mech.set_contact_data(theta.detach().cpu().numpy())      # (waits for the handle's work in flight: the table is mechanism data)
        dev = z0.device
        Z, status, DZ, DU = _record(mech, H, dev)
        DC = torch.empty((H, B, 5 * Nc, s.nx), dtype=dt, device=dev) if Nc else None
        api._chk(api.lib().dojo_rollout_data_record_dev(mech.h, api.addr(z0c), api.addr(Uc), H, api.addr(Z), api.addr(status), api.addr(DZ), api.addr(DU), api.addr(DC), api.torch_stream(dev)))
        ctx.mech, ctx.H, ctx.has_u, ctx.theta_device, ctx.layout = mech, H, U is not None, theta.device, (DU is not None, DC is not None)
        ctx.save_for_backward(z0c, Z, status, DZ, *[t for t in (DU, DC) if t is not None])
        ctx.mark_non_differentiable(status)
        return Z, status

    @staticmethod
    def backward(ctx, gZ, _gstatus):
        mech, H = ctx.mech, ctx.H
        s, B = mech.spec, mech.batch
        Nc = len(s.contacts)
        z0, Z, status, DZ = ctx.saved_tensors[:4]
        rest = list(ctx.saved_tensors[4:])
        DU = rest.pop(0) if ctx.layout[0] else None
        DC = rest.pop(0) if ctx.layout[1] else None
        gZ, = _cotangents(Z, gZ)
        need = ctx.needs_input_grad                    # (mech, z0, U, theta, steps)
        want_u = ctx.has_u and s.nu > 0 and need[2]
        gU = torch.empty((H, B, s.nu), dtype=Z.dtype, device=Z.device) if want_u else None
        gz = torch.empty((B, s.nx), dtype=Z.dtype, device=Z.device) if need[1] else None
        gth = torch.empty((Nc, 5), dtype=Z.dtype, device=Z.device) if (need[3] and Nc) else None
        if gth is not None or gz is not None:
            api._chk(api.lib().dojo_rollout_data_adjoint_dev(mech.h, H, api.addr(DZ), api.addr(DC), api.addr(gZ), 1, api.addr(Z), api.addr(status), None, api.addr(gth), api.addr(gz), api.torch_stream(Z.device)))
        if gU is not None:
            api._chk(api.lib().dojo_rollout_adjoint_dev(mech.h, H, api.addr(DZ), api.addr(DU), api.addr(gZ), 1, api.addr(Z), api.addr(status), api.addr(gU), None, api.torch_stream(Z.device)))
        if need[3] and gth is None:
            gth = torch.zeros((0, 5), dtype=Z.dtype, device=Z.device)
        return None, (lift_tangent(gz, z0) if gz is not None else None), gU, (gth.double().to(ctx.theta_device) if need[3] else None), None


def differentiable_data_rollout(mech, z0, U, theta, steps=None):
    """-> Z [H,B,13Nb], the states after every step of the rollout from z0 under the controls U [H,B,nu] (None with `steps`) with the contact data
    theta [Nc,5] = [friction_coefficient, contact_radius, contact_origin(3)] per contact (fp64, CPU or device; shared by the batch), as a node of
    torch's graph.  Forward: `mech.set_contact_data(theta)`, then dojo_rollout_data_record_dev into torch-owned tensors (the Jacobians of every step,
    H B nx (nx + nu + 5 Nc) scalars, live as long as the graph).  Backward: dojo_rollout_data_adjoint_dev for theta (summed over the batch) and z0,
    dojo_rollout_adjoint_dev over the same record for U.  z0's gradient is lifted to state shape as in differentiable_rollout; nothing flows
    through a failed step.  Z.status [H,B] (int32, non-differentiable) is the solver status of every step."""
    Z, status = _DataRollout.apply(mech, z0, U, theta, steps)
    Z.status = status
    return Z


# The two policies of a closed-loop rollout, as _ClosedLoopRollout sees them: how the parameter tensors are checked, the policy struct of the ABI, and the
# recording and sweeping entries (nh: the hidden units whose activations are recorded, None = the entries have no ACT)
class _Affine:
    nh = None

    def check(self, params, dt, B, nobs):
        W, bias = params
        if W is None or W.dim() not in (2, 3):
            raise ValueError("W must be [na, nobs] or [B, na, nobs]")
        self.per_env, self.na = W.dim() == 3, int(W.shape[-2])
        lead = (B,) if self.per_env else ()
        return _want(W, "W", dt, [lead + (self.na, nobs)]), _want(bias, "bias", dt, [lead + (self.na,)])

    def struct(self, W, mean, scale, U_ff, act_off, bias=None):
        return api.DojoPolicy(api.addr(W), api.addr(bias), api.addr(mean), api.addr(scale), api.addr(U_ff), int(self.per_env), int(act_off), self.na, 0, 0, 0)

    def record(self, h, z0, pol, H, Z, OBS, U, ACT, *rest):
        return api.lib().dojo_rollout_policy_record_dev(h, z0, pol, H, Z, OBS, U, *rest)

    def sweep(self, h, pol, H, DZ, DU, OBS, ACT, rest, stream):
        a = api.DojoPolicyAdjoint(DZ, DU, OBS, *rest, 1, 0)
        return api.lib().dojo_rollout_policy_adjoint_dev(h, pol, H, C.byref(a), stream)


class _Mlp:
    def __init__(self, widths):
        self.widths = [int(n) for n in widths]
        self.P, self.nh = api.mlp_sizes(self.widths)

    def check(self, params, dt, B, nobs):
        theta, = params
        if theta is None or theta.dim() not in (1, 2):
            raise ValueError("theta must be [P] or [B, P]")
        self.per_env = theta.dim() == 2
        return _want(theta, "theta", dt, [(B, self.P) if self.per_env else (self.P,)]),

    def struct(self, theta, mean, scale, U_ff, act_off):
        return api.mlp_policy_struct(api.addr(theta), api.addr(mean), api.addr(scale), api.addr(U_ff), self.per_env, act_off, self.widths)

    def record(self, h, z0, pol, H, Z, OBS, U, ACT, *rest):
        return api.lib().dojo_rollout_mlp_record_dev(h, z0, pol, H, Z, OBS, U, ACT, *rest)

    def sweep(self, h, pol, H, DZ, DU, OBS, ACT, rest, stream):
        a = api.DojoMlpAdjoint(DZ, DU, OBS, ACT, *rest, 1, 0)
        return api.lib().dojo_rollout_mlp_adjoint_dev(h, pol, H, C.byref(a), stream)


class _ClosedLoopRollout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mech, policy, z0, U_ff, steps, mean, scale, act_off, *params):
        s, B, dt = mech.spec, mech.batch, _dtype(mech)
        nobs = 2 * s.nu
        z0c = _want(z0, "z0", dt, [(B, s.nz)])
        params = policy.check(params, dt, B, nobs)
        mc, sc = _want(mean, "mean", dt, [(nobs,)]), _want(scale, "scale", dt, [(nobs,)])
        H, Uc = _horizon(U_ff, "U_ff", steps, dt, B, s.nu)
        dev = z0.device
        Z, status, DZ, DU, OBS, U = _record(mech, H, dev, closed_loop=True)
        ACT = None if policy.nh is None else torch.empty((H, B, policy.nh), dtype=torch.float64, device=dev)
        pol = policy.struct(params[0], mc, sc, Uc, act_off, *params[1:])
        api._chk(policy.record(mech.h, api.addr(z0c), C.byref(pol), H, api.addr(Z), api.addr(OBS), api.addr(U), api.addr(ACT), api.addr(status), api.addr(DZ), api.addr(DU), api.torch_stream(dev)))
        ctx.mech, ctx.policy, ctx.H, ctx.act_off, ctx.has_uff = mech, policy, H, int(act_off), U_ff is not None
        optional = (ACT, mc, sc) + tuple(params[1:])
        ctx.has = [t is not None for t in optional]
        ctx.save_for_backward(z0c, params[0], Z, OBS, status, DZ, DU, *[t for t in optional if t is not None])
        ctx.mark_non_differentiable(status)
        return Z, OBS, U, status

    @staticmethod
    def backward(ctx, gZ, gOBS, gU_out, _gstatus):
        mech, policy, H = ctx.mech, ctx.policy, ctx.H
        s, B = mech.spec, mech.batch
        z0, theta, Z, OBS, status, DZ, DU = ctx.saved_tensors[:7]
        rest = list(ctx.saved_tensors[7:])
        ACT, mean, scale, *others = [rest.pop(0) if has else None for has in ctx.has]
        dt, dev = Z.dtype, Z.device
        gZ, gOBS, gU_out = _cotangents(Z, gZ, gOBS, gU_out)
        need = ctx.needs_input_grad                    # (mech, policy, z0, U_ff, steps, mean, scale, act_off, *params)
        gparams = [torch.empty_like(t) if (t is not None and n) else None for t, n in zip([theta] + others, need[8:])]
        gU = torch.empty((H, B, s.nu), dtype=dt, device=dev) if (ctx.has_uff and need[3]) else None
        gz = torch.empty((B, s.nx), dtype=dt, device=dev) if need[2] else None
        pol = policy.struct(theta, mean, scale, None, ctx.act_off)
        record = [api.addr(status), api.addr(z0), api.addr(Z), None, api.addr(gZ), api.addr(gU_out), api.addr(gOBS)]      # .., M = None: computed from z0 and Z
        api._chk(policy.sweep(mech.h, C.byref(pol), H, api.addr(DZ), api.addr(DU), api.addr(OBS), api.addr(ACT) if ACT is not None and ACT.numel() else None,
                              record + [api.addr(g) for g in gparams + [gU, gz]], api.torch_stream(dev)))
        return (None, None, (lift_tangent(gz, z0) if gz is not None else None), gU, None, None, None, None) + tuple(gparams)


def differentiable_policy_rollout(mech, z0, W, bias=None, U_ff=None, steps=None, mean=None, scale=None, act_off=0):
    """-> (Z [H,B,13Nb], OBS [H+1,B,2nu], U [H,B,nu]): the closed-loop rollout from z0 under u_k = U_ff[k] + E (bias + W ((o_k - mean) .* scale)) as a node of
    torch's graph (W [na,nobs] shared or [B,na,nobs] per environment; H from U_ff, else `steps`).  Forward: dojo_rollout_policy_record_dev into
    torch-owned tensors; backward: ONE dojo_rollout_policy_adjoint_dev call with the cotangents of all three outputs.  Gradients flow to z0 (lifted
    to state shape as in differentiable_rollout), W, bias and U_ff; mean and scale are frozen.  A shared W receives the sum over the batch.
    Z.status [H,B] (int32, non-differentiable) is the solver status of every step; nothing flows through a failed step's Jacobians."""
    Z, OBS, U, status = _ClosedLoopRollout.apply(mech, _Affine(), z0, U_ff, steps, mean, scale, act_off, W, bias)
    Z.status = status
    return Z, OBS, U


def differentiable_mlp_rollout(mech, z0, theta, widths, U_ff=None, steps=None, mean=None, scale=None, act_off=0):
    """-> (Z [H,B,13Nb], OBS [H+1,B,2nu], U [H,B,nu]): the closed-loop rollout from z0 under the tanh network of include/dojo_hip.h `DojoMlpPolicy` as a node of
    torch's graph.  theta is ONE flat tensor, [P] (shared) or [B, P] (one policy per environment), in the layout of api.pack_mlp -- layer after layer the
    row-major weight, then the bias -- so that the parameters of a torch.nn module reach it through torch.cat; widths = [n_0 = 2 nu, .., n_L = na].
    Forward: dojo_rollout_mlp_record_dev into torch-owned tensors (the activations ACT are saved for backward beside DZ and DU); backward: ONE
    dojo_rollout_mlp_adjoint_dev call with the cotangents of all three outputs.  Gradients flow to z0 (lifted to state shape as in
    differentiable_rollout), theta and U_ff; mean and scale are frozen.  A shared theta receives the sum over the batch.  Z.status [H,B] (int32,
    non-differentiable) is the solver status of every step; nothing flows through a failed step's Jacobians."""
    Z, OBS, U, status = _ClosedLoopRollout.apply(mech, _Mlp(widths), z0, U_ff, steps, mean, scale, act_off, theta)
    Z.status = status
    return Z, OBS, U
