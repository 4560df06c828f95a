"""DojoEnvironments' `Environment` API (DojoEnvironments/src/environments.jl:60-110) for B copies of an environment on
one GPU: `step`, `get_state`, `state_map`, `input_map` of `AntARS` (environments/ant_ars.jl) and `QuadrupedSampling`
(environments/quadruped_sampling.jl).  States, inputs and observations are torch tensors on the device; every call
enqueues kernels of libdojo_hip.so on torch's current stream and returns without synchronizing, so a sampling loop
(observation -> policy -> step -> reward) never touches the host."""
import ctypes as C
import numpy as np
from . import api
from .coords import nominal_minimal
from .mechanisms import get_mechanism
from .topology import SolverOptions

# environment -> (mechanism, contact forces in the observation, unactuated leading inputs)
_ENVIRONMENTS = {"ant_ars": ("ant", True, 6), "quadruped_sampling": ("quadruped", False, 6)}


class BatchedEnvironment:
    def __init__(self, name, batch, dtype="f32", device=0, opts=None, **mechanism_kwargs):
        import torch
        mech, self.contact_forces, self.n_unactuated = _ENVIRONMENTS[name]
        self.name = name
        self.spec = get_mechanism(mech, **mechanism_kwargs)
        self.batch = int(batch)
        self.device = torch.device("cuda", device)
        self.mechanism = api.BatchedMechanism(self.spec, batch, dtype=dtype, device=device, opts=opts or SolverOptions())
        self.torch_dtype = torch.float32 if self.mechanism.np_dtype == np.float32 else torch.float64
        self.nx = 2 * self.spec.nu
        self.nobs = self.nx + (len(self.spec.contacts) if self.contact_forces else 0)
        self.status = torch.zeros(self.batch, dtype=torch.int32, device=self.device)
        self.iters = torch.zeros(self.batch, dtype=torch.int32, device=self.device)
        self._x = torch.zeros(self.batch, self.nx, dtype=self.torch_dtype, device=self.device)      # minimal state after the last step
        self._stepped = False

    # ---- ant_ars.jl:53-61, quadruped_sampling.jl:51-58 ----
    def state_map(self, state):
        return state[:, :self.nx]

    def input_map(self, inp):
        import torch
        return torch.cat([torch.zeros(self.batch, self.n_unactuated, dtype=self.torch_dtype, device=self.device), inp.to(self.torch_dtype)], dim=1)

    def initialize(self, x0=None, **kw):
        """initialize!(environment, model; kwargs...) (environments.jl:112-114): every copy at the mechanism's nominal state
        (keywords as the reference's initialize_<model>!), or at the given minimal states x0 [B, 2nu]."""
        import torch
        if x0 is None:
            x0 = np.tile(nominal_minimal(self.spec, **kw), (self.batch, 1))
        self._x = torch.as_tensor(x0, dtype=self.torch_dtype).to(self.device).reshape(self.batch, self.nx).contiguous()
        self._stepped = False
        return self._x

    def step(self, state, inp):
        """step!(environment, state, input) (environments.jl:77-84): step_minimal_coordinates! of state_map(state), input_map(input)."""
        import torch
        x = self.state_map(state).to(self.torch_dtype).contiguous()
        u = self.input_map(inp).contiguous()
        xn = torch.empty_like(x)
        api._chk(api.lib().dojo_step_minimal_dev(self.mechanism.h, api.addr(x), api.addr(u), api.addr(xn),
                                                 api.addr(self.status), api.addr(self.iters), api.torch_stream(self.device)))
        self._x = xn
        self._stepped = True
        self._keep = (x, u)                                     # inputs of kernels still in flight
        return xn

    def get_state(self):
        """get_state(environment): minimal state (+ clamped contact normal impulses for AntARS, ant_ars.jl:72-80)."""
        import torch
        if not self._stepped:        # a freshly built ContactConstraint holds the neutral vector [1,1,0,0] (contacts/constructor.jl:38-39)
            obs = torch.ones(self.batch, self.nobs, dtype=self.torch_dtype, device=self.device)
            obs[:, :self.nx] = self._x
            return obs
        obs = torch.empty(self.batch, self.nobs, dtype=self.torch_dtype, device=self.device)
        api._chk(api.lib().dojo_observe_dev(self.mechanism.h, None, api.addr(obs), int(self.contact_forces), api.torch_stream(self.device)))
        return obs

    def rollout_policy(self, theta, horizon, mean=None, scale=None, U_ff=None):
        """`horizon` steps under the linear policy action = theta ((observation - mean) .* scale) in ONE call (dojo_rollout_policy_dev): the policy is
        evaluated on the device between the steps, the environment groups run chained on the library's streams and are joined into torch's current
        stream at the end.  theta [na, nobs] (shared) or [B, na, nobs] (one policy per environment), na = nu - n_unactuated actions behind the
        unactuated leading inputs; mean, scale [nobs] or None; U_ff [horizon, B, nu] or None (feed-forward term).  Starts from the minimal state of
        `initialize()`.  Returns (OBS [horizon + 1, B, nobs], U [horizon, B, nu], status [horizon, B]) as device tensors, without synchronizing:
        OBS[k] is get_state before step k (contact entries of OBS[0]: the neutral 1.0), OBS[horizon] that of the final state.

        This is the reference's simulate!(mechanism, steps, storage, control!) (src/simulation/simulate.jl:16-37): the state is carried in MAXIMAL
        coordinates from step to step.  The stepwise `step` re-projects through minimal coordinates at every step (step_minimal_coordinates!), as
        DojoEnvironments' step! does; the two agree to the accuracy of the joint constraints, not bit for bit."""
        import torch
        B, nu = self.batch, self.spec.nu
        H, na = int(horizon), nu - self.n_unactuated
        dev = lambda t, shape: None if t is None else torch.as_tensor(t, device=self.device).to(self.torch_dtype).reshape(shape).contiguous()
        theta = torch.as_tensor(theta, device=self.device).to(self.torch_dtype).contiguous()
        per_env = theta.dim() == 3
        if tuple(theta.shape) != ((B, na, self.nobs) if per_env else (na, self.nobs)):
            raise ValueError("theta must be [%d, %d] or [%d, %d, %d], got %s" % (na, self.nobs, B, na, self.nobs, tuple(theta.shape)))
        mean, scale, U_ff = dev(mean, (self.nobs,)), dev(scale, (self.nobs,)), dev(U_ff, (H, B, nu))
        x0 = self._x.contiguous()
        z0 = torch.empty(B, 13 * self.spec.Nb, dtype=self.torch_dtype, device=self.device)
        L, h = api.lib(), self.mechanism.h
        api._chk(L.dojo_minimal_to_maximal_dev(h, api.addr(x0), api.addr(z0), api.torch_stream(self.device)))
        OBS = torch.empty(H + 1, B, self.nobs, dtype=self.torch_dtype, device=self.device)
        U = torch.empty(H, B, nu, dtype=self.torch_dtype, device=self.device)
        status = torch.empty(H, B, dtype=torch.int32, device=self.device)
        pol = api.DojoPolicy(api.addr(theta), None, api.addr(mean), api.addr(scale), api.addr(U_ff), int(per_env), self.n_unactuated, na, int(self.contact_forces), 0, 0)
        api._chk(L.dojo_rollout_policy_dev(h, api.addr(z0), C.byref(pol), H, None, api.addr(OBS), api.addr(U),
                                           api.addr(status), api.torch_stream(self.device)))
        self._keep = (x0, z0, theta, mean, scale, U_ff)          # inputs of kernels still in flight
        self._stepped = True
        return OBS, U, status

    def close(self):
        self.mechanism.close()
