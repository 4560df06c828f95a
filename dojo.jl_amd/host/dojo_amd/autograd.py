"""Rollouts as a differentiable torch operation (torch is plumbing only: it owns the buffers and the graph; the rollout, the IFT
Jacobians and the reverse sweep are the library's kernels, include/dojo_hip.h "Reverse-mode rollouts").

    Z = differentiable_rollout(mech, z0, U)          # z0 [B,13Nb], U [H,B,nu] device tensors -> Z [H,B,13Nb]
    loss(Z).backward()                               # U.grad [H,B,nu], z0.grad [B,13Nb]

Everything is enqueued on torch's current stream and nothing synchronizes.  The gradient is the chain of the handle's gradient mode:
set `mech.set_gradient_mode(api.GRAD_CONSISTENT)` for the derivative of the rollout.
"""
import ctypes as C

import torch

from . import api


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def lift_tangent(gz, z0):
    """[B,nx] tangent cotangent -> [B,13Nb] state cotangent at z0: g_x, g_v, g_omega are copied and g_q = q0 (x) (0, g_phi), the transpose's
    right inverse on the tangent space of the unit sphere at q0 (a 4-byte z0 stands for q0 / |q0|, as in the kernels)."""
    B = z0.shape[0]
    g = gz.double().reshape(B, -1, 12); z = z0.double().reshape(B, -1, 13)
    q = z[..., 6:10]; q = q / q.norm(dim=-1, keepdim=True) if z0.dtype == torch.float32 else q
    s, v, p = q[..., :1], q[..., 1:], g[..., 6:9]
    gq = torch.cat([-(v * p).sum(-1, keepdim=True), s * p + torch.linalg.cross(v, p)], -1)
    return torch.cat([g[..., 0:6], gq, g[..., 9:12]], -1).reshape(B, -1).to(z0.dtype)


class _Rollout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mech, z0, U, steps):
        s, B = mech.spec, mech.batch
        dt = torch.float32 if mech.dtype_code == 1 else torch.float64
        if not z0.is_cuda or z0.dtype != dt or tuple(z0.shape) != (B, s.nz):
            raise ValueError("z0 must be a %s device tensor of shape %s" % (dt, (B, s.nz)))
        if U is not None and s.nu:
            if not U.is_cuda or U.dtype != dt or U.dim() != 3 or tuple(U.shape[1:]) != (B, s.nu):
                raise ValueError("U must be a %s device tensor of shape (H, %d, %d)" % (dt, B, s.nu))
            H = int(U.shape[0]); Uc = U.contiguous()
        else:
            H = int(steps); Uc = None
        dev = z0.device; z0c = z0.contiguous()
        Z = torch.empty((H, B, s.nz), dtype=dt, device=dev)
        status = torch.empty((H, B), dtype=torch.int32, device=dev)
        DZ = torch.empty((H, B, s.nx, s.nx), dtype=dt, device=dev)          # the record: freed with the graph
        DU = torch.empty((H, B, s.nu, s.nx), dtype=dt, device=dev) if s.nu else None
        api._chk(api.lib().dojo_rollout_record_dev(mech.h, _ptr(z0c), _ptr(Uc), H, _ptr(Z), _ptr(status), _ptr(DZ), _ptr(DU), _stream(dev)))
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
        gZ = gZ.contiguous()
        want_u = ctx.has_u and s.nu > 0 and ctx.needs_input_grad[2]
        gU = torch.empty((H, B, s.nu), dtype=Z.dtype, device=Z.device) if want_u else None
        gz = torch.empty((B, s.nx), dtype=Z.dtype, device=Z.device) if ctx.needs_input_grad[1] else None
        api._chk(api.lib().dojo_rollout_adjoint_dev(mech.h, H, _ptr(DZ), _ptr(DU), _ptr(gZ), 1, _ptr(Z), _ptr(status), _ptr(gU), _ptr(gz), _stream(Z.device)))
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
