"""The host-pointer entries of the single-step and coordinate half of the C ABI against their device entries, and the refusal of mechanisms with a
kinematic loop by every entry that works in minimal coordinates.

1. Host entry equals device entry.  Two handles of one mechanism get the same sequence of calls, one through host pointers (upload, the device entry,
   download: the staging of dojo.jl_amd/csrc/dojo_hip.hip) and one through the `_dev` entries on torch tensors.  The kernels are the same, so every output
   is equal bit for bit -- status and iters included -- and dojo_get_state of the host handle is the state the device entries left behind.
   Shapes: the cartpole at B = 129 (Nb = 2: 258 (environment, body) threads, the first batch past one 256-thread block of the per-body kernels) and the
   sphere, the smallest mechanism with inputs and a contact, at B = 65 (past the 64-thread block of min2max_kernel); fp64 and fp32 handles.
2. Loop refusals.  On the four-bar linkage every such entry (the closed-loop rollouts and the Riccati pass through their shared refusals) returns
   DOJO_ERR_UNSUPPORTED with its own text, launches nothing and leaves the handle usable."""
import ctypes as C

import numpy as np
import pytest
import torch

import dojo_amd as d
from dojo_amd import api
from gpu_util import assert_same, dev, host

pytestmark = pytest.mark.gpu

UNSUPPORTED = -2
CASES = [("cartpole", 129), ("sphere", 65)]


def _state(gm):
    z = np.empty((gm.batch, gm.spec.nz), gm.np_dtype)
    api._chk(api.lib().dojo_get_state(gm.h, api.addr(z)))
    return z


class Dev:
    """the `_dev` entries of a handle on torch tensors; outputs start as NaN / -77 so that an entry the device does not write shows.  Every input tensor is
    held in a local until the device is through with it: a tensor dropped earlier hands its memory to the next allocation."""

    def __init__(self, gm):
        self.gm, self.L, self.B, self.s = gm, api.lib(), gm.batch, gm.spec
        self.tdt = torch.float32 if gm.dtype_code else torch.float64

    def new(self, *shape, dtype=None):
        return torch.full(shape, float("nan"), dtype=dtype or self.tdt, device="cuda")

    def ints(self):
        return torch.full((self.B,), -77, dtype=torch.int32, device="cuda")

    def step(self, z, u, with_gradient):
        s, B = self.s, self.B
        zn, st, it = self.new(B, s.nz), self.ints(), self.ints()
        dz = self.new(B, s.nx, s.nx) if with_gradient else None
        du = self.new(B, max(s.nu, 1), s.nx) if with_gradient else None
        self.keep = (dev(z), dev(u))                      # dojo_contact_gradients_dev re-linearizes at them
        api._chk(self.L.dojo_step_dev(self.gm.h, api.addr(self.keep[0]), api.addr(self.keep[1]), api.addr(zn), api.addr(st), api.addr(it), api.addr(dz), api.addr(du), api.torch_stream()))
        self.zn = zn
        return zn, st, it, dz, du

    def contact_gradients(self):
        dc = self.new(self.B, 5 * len(self.s.contacts), self.s.nx)
        api._chk(self.L.dojo_contact_gradients_dev(self.gm.h, api.addr(self.keep[0]), api.addr(self.keep[1]), api.addr(dc), api.torch_stream()))
        return dc

    def step_impulses(self, z, jf):
        """what dojo_step_impulses does: the impulses, divided by the time step in fp64, in the external-force slot of a step without controls"""
        s, B = self.s, self.B
        folded = (torch.zeros(B, 6 * s.Nb, dtype=torch.float64, device="cuda") + dev(jf).double() * (1.0 / s.timestep)).to(self.tdt)
        zn, st, it = self.new(B, s.nz), self.ints(), self.ints()
        zd = dev(z)
        api._chk(self.L.dojo_set_external_force_dev(self.gm.h, api.addr(folded)))
        api._chk(self.L.dojo_step_dev(self.gm.h, api.addr(zd), None, api.addr(zn), api.addr(st), api.addr(it), None, None, api.torch_stream()))
        torch.cuda.synchronize()
        api._chk(self.L.dojo_set_external_force_dev(self.gm.h, None))
        self.zn = zn
        return zn, st, it

    def coords(self, a, to_max):
        out = self.new(self.B, self.s.nz if to_max else 2 * self.s.nu)
        f = self.L.dojo_minimal_to_maximal_dev if to_max else self.L.dojo_maximal_to_minimal_dev
        ad = dev(a)
        api._chk(f(self.gm.h, api.addr(ad), api.addr(out), api.torch_stream()))
        torch.cuda.synchronize()
        return out

    def step_minimal(self, x, u, jac):
        s, B, nm = self.s, self.B, 2 * self.s.nu
        xn, st, it = self.new(B, nm), self.ints(), self.ints()
        xd, ud = dev(x), dev(u)
        if not jac:
            api._chk(self.L.dojo_step_minimal_dev(self.gm.h, api.addr(xd), api.addr(ud), api.addr(xn), api.addr(st), api.addr(it), api.torch_stream()))
            torch.cuda.synchronize()
            return xn, st, it
        jx, ju = self.new(B, nm, nm), self.new(B, nm, s.nu)
        api._chk(self.L.dojo_minimal_gradients_dev(self.gm.h, api.addr(xd), api.addr(ud), api.addr(xn), api.addr(st), api.addr(it), api.addr(jx), api.addr(ju), api.torch_stream()))
        torch.cuda.synchronize()
        return xn, st, it, jx, ju

    def observe(self, contact_forces):
        obs = self.new(self.B, 2 * self.s.nu + (len(self.s.contacts) if contact_forces else 0))
        api._chk(self.L.dojo_observe_dev(self.gm.h, api.addr(self.zn), api.addr(obs), int(contact_forces), api.torch_stream()))
        return obs

    def next_state(self, z):
        zo, zd = self.new(self.B, self.s.nz), dev(z)
        api._chk(self.L.dojo_next_state_dev(self.gm.h, api.addr(zd), api.addr(zo), api.torch_stream()))
        torch.cuda.synchronize()
        return zo

    def observation_jacobian(self, z):
        M, zd = self.new(self.B, 2 * self.s.nu, 24, dtype=torch.float64), dev(z)
        api._chk(self.L.dojo_observation_jacobian_dev(self.gm.h, api.addr(zd), 1, api.addr(M), api.torch_stream()))
        torch.cuda.synchronize()
        return M

    def simulate(self, z0, U):
        H, s, B = U.shape[0], self.s, self.B
        Z, S, st = self.new(H, B, s.nz), self.new(H, B, s.Nb, 25), torch.full((H, B), -77, dtype=torch.int32, device="cuda")
        zd, Ud = dev(z0), dev(U)
        api._chk(self.L.dojo_simulate_dev(self.gm.h, api.addr(zd), api.addr(Ud), H, api.addr(Z), api.addr(S), api.addr(st), api.torch_stream()))
        torch.cuda.synchronize()
        return Z, S, st


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name,B", CASES)
def test_host_entries_equal_the_device_entries(name, B, dtype):
    spec = d.get_mechanism(name)
    assert spec.nu > 0 and (name != "sphere" or len(spec.contacts) == 1)
    Nc = len(spec.contacts)
    Z, U = d.synthetic_inputs(spec, B)
    gh = api.BatchedMechanism(spec, B, dtype=dtype)
    gd = api.BatchedMechanism(spec, B, dtype=dtype)
    dev = Dev(gd)
    try:
        Z, U = Z.astype(gh.np_dtype), U.astype(gh.np_dtype)
        # dojo_step with gradients, then dojo_gradients and dojo_contact_gradients (host layout: row-major; device layout: column-major per environment)
        zn, st, it = gh.step(Z, U, with_gradient=True)
        dzn, dst, dit, ddz, ddu = dev.step(Z, U, True)
        assert (st == 0).any() and np.isfinite(zn[st == 0]).all()
        assert_same("step z_next", zn, host(dzn)); assert_same("step status", st, host(dst)); assert_same("step iters", it, host(dit))
        assert_same("step get_state", _state(gh), zn)
        dz, du = gh.gradients()
        assert_same("gradients dz", dz, host(ddz).transpose(0, 2, 1)); assert_same("gradients du", du, host(ddu)[:, :spec.nu].transpose(0, 2, 1))
        if Nc:
            assert_same("contact_gradients", gh.contact_gradients(), host(dev.contact_gradients()).transpose(0, 2, 1))
        assert_same("contact_gradients get_state", _state(gh), zn)
        # dojo_observe reads the state and the impulses that step left on the handle
        for cf in (False, True):
            assert_same("observe %d" % cf, gh.observe(cf), host(dev.observe(cf)))
        assert_same("observe get_state", _state(gh), zn)
        # the entries that work on the caller's arrays alone
        assert_same("next_state", gh.next_state(zn), host(dev.next_state(zn)))
        assert_same("observation_jacobian", gh.observation_jacobian(zn), host(dev.observation_jacobian(zn)))
        X = gh.maximal_to_minimal(Z)
        assert_same("maximal_to_minimal", X, host(dev.coords(Z, False)))
        assert_same("minimal_to_maximal", gh.minimal_to_maximal(X), host(dev.coords(X, True)))
        assert_same("coordinate entries get_state", _state(gh), zn)
        # dojo_step_impulses
        jf = (0.01 * np.random.default_rng(5).standard_normal((B, 6 * spec.Nb))).astype(gh.np_dtype)
        zi, st, it = gh.step_impulses(zn, jf)
        dzi, dst, dit = dev.step_impulses(zn, jf)
        assert_same("step_impulses z_next", zi, host(dzi)); assert_same("step_impulses status", st, host(dst)); assert_same("step_impulses iters", it, host(dit))
        assert_same("step_impulses get_state", _state(gh), zi)
        # dojo_step_minimal, dojo_minimal_gradients in both modes: the device entries leave the maximal state on the handle as well
        xn, st, it = gh.step_minimal(X, U)
        dxn, dst, dit = dev.step_minimal(X, U, False)
        assert_same("step_minimal x_next", xn, host(dxn)); assert_same("step_minimal status", st, host(dst)); assert_same("step_minimal iters", it, host(dit))
        assert_same("step_minimal get_state", _state(gh), _state(gd))
        for mode in (0, 1):
            gh.set_gradient_mode(mode); gd.set_gradient_mode(mode)
            xn, st, it, jx, ju = gh.minimal_gradients(X, U)
            dxn, dst, dit, djx, dju = dev.step_minimal(X, U, True)
            for what, a, b in (("x_next", xn, dxn), ("status", st, dst), ("iters", it, dit), ("jx", jx, djx), ("ju", ju, dju)):
                assert_same("minimal_gradients mode %d %s" % (mode, what), a, host(b))
            assert_same("minimal_gradients get_state", _state(gh), _state(gd))
            assert np.isfinite(jx[st == 0]).all() and np.isfinite(ju[st == 0]).all()
        # dojo_simulate: states, Storage rows and status of two steps
        Us = np.stack([U, -U])
        Zs, S, sts = gh.simulate(Z, Us)
        dZs, dS, dsts = dev.simulate(Z, Us)
        assert_same("simulate Z", Zs, host(dZs)); assert_same("simulate storage", S, host(dS)); assert_same("simulate status", sts, host(dsts))
        assert_same("simulate get_state", _state(gh), Zs[-1])
    finally:
        gh.close(); gd.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_plain_integer_addresses(dtype):
    """the handle, every pointer and the stream given as plain Python ints reach the library as the 64-bit values they are: three `_dev` entries write bit for
    bit what they write for the same values wrapped in c_void_p (without argtypes ctypes would pass an int as a 32-bit C int)"""
    spec, B, H = d.get_mechanism("cartpole"), 3, 2
    L = api.lib()
    entries = (L.dojo_maximal_to_minimal_dev, L.dojo_next_state_dev, L.dojo_rollout_record_dev)
    assert all(f.argtypes and all(t is not None for t in f.argtypes) for f in entries)
    Z0, U0 = d.synthetic_inputs(spec, B)
    gm = api.BatchedMechanism(spec, B, dtype=dtype)
    try:
        tdt = torch.float32 if gm.dtype_code else torch.float64
        z, U = dev(Z0, tdt), dev(np.stack([U0, -U0]), tdt)
        nan = lambda *shape: torch.full(shape, float("nan"), dtype=tdt, device="cuda")
        outs = []
        for wrap in (int, C.c_void_p):
            a = lambda t: wrap(t.data_ptr())
            h, stream = wrap(gm.h.value), wrap(api.torch_stream())
            x, zo, Z, DZ, DU = nan(B, 2 * spec.nu), nan(B, spec.nz), nan(H, B, spec.nz), nan(H, B, spec.nx, spec.nx), nan(H, B, spec.nu, spec.nx)
            st = torch.full((H, B), -77, dtype=torch.int32, device="cuda")
            api._chk(L.dojo_maximal_to_minimal_dev(h, a(z), a(x), stream))
            api._chk(L.dojo_next_state_dev(h, a(z), a(zo), stream))
            api._chk(L.dojo_rollout_record_dev(h, a(z), a(U), H, a(Z), a(st), a(DZ), a(DU), stream))
            outs.append([host(t) for t in (x, zo, Z, st, DZ, DU)])
        assert np.isfinite(outs[0][0]).all() and np.isfinite(outs[0][1]).all() and (outs[0][3] == 0).any()      # the entries ran and wrote
        for what, got, ref in zip(("x", "z_out", "Z", "status", "DZ", "DU"), *outs):
            assert_same(what, got, ref)
    finally:
        gm.close()


# the texts are the literals of the entries' source
_LOOP = "the minimal coordinates of a mechanism with a kinematic loop are not those of a tree traversal"
_LONG = ": " + _LOOP + " (the reference sets them with exclude_ids): not supported"
_SHORT = ": " + _LOOP + ": not supported"
LOOP_REFUSALS = [("dojo_rollout_policy_dev", _LONG), ("dojo_riccati_dev", _LONG), ("dojo_observation_jacobian_dev", _SHORT), ("dojo_observation_jacobian", _SHORT),
                 ("dojo_minimal_to_maximal_dev", _LONG), ("dojo_maximal_to_minimal_dev", _LONG), ("dojo_observe_dev", _LONG), ("dojo_step_minimal_dev", _LONG),
                 ("dojo_minimal_gradients_dev", _LONG), ("dojo_rollout_mlp_dev", _LONG)]


def test_loop_refusals():
    spec = d.get_fourbar()
    assert spec.nu > 0
    gm = api.BatchedMechanism(spec, 1, dtype="f64")
    L = api.lib()
    try:
        buf = torch.zeros(4096, dtype=torch.float64, device="cuda"); ibuf = torch.zeros(16, dtype=torch.int32, device="cuda")
        hbuf = np.zeros(4096)
        p, ip, st = api.addr(buf), api.addr(ibuf), api.torch_stream()
        pol = api.DojoPolicy(buf.data_ptr(), None, None, None, None, 1, 0, 1, 0, 0, 0)
        mlp = api.mlp_policy_struct(buf.data_ptr(), None, None, None, 1, 0, [2 * spec.nu, 1])
        ric = api.DojoRiccati()
        for k in ("A", "Bm", "lx", "lu", "lxx", "luu", "K", "kff"):
            setattr(ric, k, buf.data_ptr())
        ric.fail = ibuf.data_ptr(); ric.na = 1; ric.act_off = 0
        calls = {"dojo_rollout_policy_dev": lambda: L.dojo_rollout_policy_dev(gm.h, p, C.byref(pol), 1, p, p, p, ip, st),
                 "dojo_rollout_mlp_dev": lambda: L.dojo_rollout_mlp_dev(gm.h, p, C.byref(mlp), 1, p, p, p, None, ip, st),
                 "dojo_riccati_dev": lambda: L.dojo_riccati_dev(gm.h, 1, C.byref(ric), st),
                 "dojo_observation_jacobian_dev": lambda: L.dojo_observation_jacobian_dev(gm.h, p, 1, p, st),
                 "dojo_observation_jacobian": lambda: L.dojo_observation_jacobian(gm.h, api.addr(hbuf), api.addr(hbuf)),
                 "dojo_minimal_to_maximal_dev": lambda: L.dojo_minimal_to_maximal_dev(gm.h, p, p, st),
                 "dojo_maximal_to_minimal_dev": lambda: L.dojo_maximal_to_minimal_dev(gm.h, p, p, st),
                 "dojo_observe_dev": lambda: L.dojo_observe_dev(gm.h, p, p, 0, st),
                 "dojo_step_minimal_dev": lambda: L.dojo_step_minimal_dev(gm.h, p, p, p, ip, ip, st),
                 "dojo_minimal_gradients_dev": lambda: L.dojo_minimal_gradients_dev(gm.h, p, p, p, ip, ip, p, p, st)}
        assert len(LOOP_REFUSALS) == 10 and sorted(calls) == sorted(e for e, _ in LOOP_REFUSALS)
        for entry, text in LOOP_REFUSALS:
            assert calls[entry]() == UNSUPPORTED, entry
            assert gm.last_error() == entry + text, (entry, gm.last_error())
        torch.cuda.synchronize()
        assert not buf.any() and not ibuf.any() and not hbuf.any()           # nothing was launched or copied
        Z, U = d.synthetic_inputs(spec, 1)
        zn, status, iters = gm.step(Z, U)
        assert np.isfinite(zn).all() and iters[0] >= 1
    finally:
        gm.close()
