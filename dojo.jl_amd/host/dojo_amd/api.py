"""ctypes binding of libdojo_hip.so + the host-side mirror of Dojo's API for the hot path.

Reference surface mirrored here (argument meaning and error behaviour follow the reference):
  step!(mechanism, z, u; opts)                 src/simulation/step.jl:11-30        -> step(mech, z, u, opts=...)
  simulate!(mechanism, steps, storage, ctrl!)  src/simulation/simulate.jl:16-36    -> simulate(mech, z0, U)
  get_maximal_gradients!(mechanism, z, u)      src/gradients/state.jl:69-76        -> get_maximal_gradients(mech, z, u)
  get_solution(mechanism)                      src/gradients/finite_difference.jl  -> mech.get_solution()
The batch axis is the leading axis of every array.  There is NO CPU fallback: if the HIP
library or a GPU is missing, construction raises.
"""
import ctypes as C
import os
# one hardware queue per environment group of dojo_rollout (must be set before the HIP runtime starts; ROCm default is 4)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "24")
import numpy as np
from .topology import CTopology, CSolverOptions, CDims, SolverOptions

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "csrc")
_LIB_PATH = os.environ.get("DOJO_HIP_LIB") or os.path.join(_CSRC, "libdojo_hip.so")   # override: instrumented builds (tools/build_variant.sh prof -DDJ_PROF)
_lib = None

STATUS_SUCCESS, STATUS_FAILED, STATUS_EXCESSIVE_W = 0, 1, 2
GRAD_REFERENCE, GRAD_CONSISTENT = 0, 1
KERNEL_FAMILIES = ("plain", "tsd", "gen", "lin", "ss")     # dojo_get_kernel_build's family codes


class DojoError(RuntimeError):
    pass


# include/dojo_hip.h, one line per entry point: the C return type and the parameters -- p: DojoHandle, any pointer (struct pointers, int32_t out[3] and
# the stream included), i: int32_t, l: int64_t, d: double.  With argtypes a plain Python int is a full 64-bit address; without, ctypes would cut it to a C int.
_KINDS = {"p": C.c_void_p, "i": C.c_int32, "l": C.c_int64, "d": C.c_double}
_SIGNATURES = {
    "dojo_device_count": (C.c_int, ""), "dojo_last_error": (C.c_char_p, ""), "dojo_handle_error": (C.c_char_p, "p"), "dojo_create": (C.c_int, "piiip"), "dojo_destroy": (None, "p"),
    "dojo_get_dims": (C.c_int, "pp"), "dojo_set_options": (C.c_int, "pp"), "dojo_set_gradient_mode": (C.c_int, "pi"), "dojo_set_refinement": (C.c_int, "pd"),
    "dojo_step": (C.c_int, "ppppppi"), "dojo_step_impulses": (C.c_int, "pppppp"), "dojo_next_state": (C.c_int, "ppp"), "dojo_next_state_dev": (C.c_int, "pppp"),
    "dojo_get_solution": (C.c_int, "pppp"), "dojo_get_mu": (C.c_int, "pp"), "dojo_get_diagnostics": (C.c_int, "pp"), "dojo_get_kernel_build": (C.c_int, "pp"),
    "dojo_gradients": (C.c_int, "ppp"), "dojo_rollout": (C.c_int, "pppipp"), "dojo_get_state": (C.c_int, "pp"), "dojo_step_dev": (C.c_int, "ppppppppp"),
    "dojo_set_async": (C.c_int, "pi"), "dojo_set_groups": (C.c_int, "pi"), "dojo_set_iteration_cap": (C.c_int, "pi"), "dojo_set_dispatch_order": (C.c_int, "pi"),
    "dojo_join": (C.c_int, "pp"), "dojo_comm_unique_id": (C.c_int, "p"), "dojo_comm_init": (C.c_int, "piip"), "dojo_allgather_dev": (C.c_int, "ppplip"),
    "dojo_comm_info": (C.c_int, "ppp"), "dojo_rollout_dev": (C.c_int, "pppippp"), "dojo_set_external_force": (C.c_int, "pp"), "dojo_set_external_force_dev": (C.c_int, "pp"),
    "dojo_simulate": (C.c_int, "pppippp"), "dojo_simulate_dev": (C.c_int, "pppipppp"), "dojo_rollout_record_dev": (C.c_int, "pppippppp"),
    "dojo_rollout_adjoint_dev": (C.c_int, "pipppippppp"), "dojo_rollout_gradients": (C.c_int, "pppipipppp"), "dojo_set_contact_data": (C.c_int, "pp"),
    "dojo_get_contact_data": (C.c_int, "pp"), "dojo_rollout_data_record_dev": (C.c_int, "pppipppppp"), "dojo_rollout_data_adjoint_dev": (C.c_int, "pipppipppppp"),
    "dojo_rollout_data_gradients": (C.c_int, "pppipipppppp"), "dojo_rollout_tangent_dev": (C.c_int, "piippppppipppp"), "dojo_rollout_tangents": (C.c_int, "pppiipppippp"),
    "dojo_rollout_policy_dev": (C.c_int, "pppippppp"), "dojo_rollout_policy": (C.c_int, "pppipppp"), "dojo_observation_jacobian_dev": (C.c_int, "ppipp"),
    "dojo_observation_jacobian": (C.c_int, "ppp"), "dojo_rollout_policy_record_dev": (C.c_int, "pppippppppp"), "dojo_rollout_policy_adjoint_dev": (C.c_int, "ppipp"),
    "dojo_rollout_policy_gradients": (C.c_int, "pppipipppppppppp"), "dojo_rollout_mlp_dev": (C.c_int, "pppipppppp"), "dojo_rollout_mlp": (C.c_int, "pppipppp"),
    "dojo_rollout_mlp_record_dev": (C.c_int, "pppipppppppp"), "dojo_rollout_mlp_adjoint_dev": (C.c_int, "ppipp"), "dojo_rollout_mlp_gradients": (C.c_int, "pppipippppppppp"),
    "dojo_riccati_dev": (C.c_int, "pipp"), "dojo_riccati": (C.c_int, "pip"), "dojo_observe": (C.c_int, "ppi"), "dojo_observe_dev": (C.c_int, "pppip"),
    "dojo_contact_gradients": (C.c_int, "pp"), "dojo_contact_gradients_dev": (C.c_int, "ppppp"), "dojo_minimal_to_maximal": (C.c_int, "ppp"),
    "dojo_maximal_to_minimal": (C.c_int, "ppp"), "dojo_step_minimal": (C.c_int, "pppppp"), "dojo_minimal_to_maximal_dev": (C.c_int, "pppp"),
    "dojo_maximal_to_minimal_dev": (C.c_int, "pppp"), "dojo_step_minimal_dev": (C.c_int, "ppppppp"), "dojo_minimal_gradients": (C.c_int, "pppppppp"),
    "dojo_minimal_gradients_dev": (C.c_int, "ppppppppp"), "dojo_last_kernel_ms": (C.c_int, "pp"), "dojo_last_kernel_times": (C.c_int, "ppp"),
    "dojo_kernel_time_totals": (C.c_int, "ppppi"),
}
EXPORTED_SYMBOLS = list(_SIGNATURES)
# include/dojo_hip_trajopt.h, the second public header, in the same notation
_TRAJOPT_SIGNATURES = {"dojo_rollout_minimal_dev": (C.c_int, "pipp"), "dojo_rollout_minimal": (C.c_int, "pip")}
TRAJOPT_SYMBOLS = list(_TRAJOPT_SIGNATURES)
# include/dojo_hip_limits.h, the third: control-limited iLQR
_LIMITS_SIGNATURES = {"dojo_riccati_box_dev": (C.c_int, "pipppppp"), "dojo_riccati_box": (C.c_int, "pippppp"),
                      "dojo_rollout_minimal_box_dev": (C.c_int, "pippp"), "dojo_rollout_minimal_box": (C.c_int, "pipp")}
LIMITS_SYMBOLS = list(_LIMITS_SIGNATURES)
# include/dojo_hip_constraints.h, the fourth: the augmented-Lagrangian terms of stage constraints in the backward pass
_CONSTRAINT_SIGNATURES = {"dojo_riccati_al_dev": (C.c_int, "pippppppp"), "dojo_riccati_al": (C.c_int, "pipppppp")}
CONSTRAINT_SYMBOLS = list(_CONSTRAINT_SIGNATURES)
# include/dojo_hip_linesearch.h, the fifth: the step lengths of a line search side by side -- the fan rollout and the selection kernel
_LINESEARCH_SIGNATURES = {"dojo_rollout_minimal_fan_dev": (C.c_int, "piippp"), "dojo_rollout_minimal_fan": (C.c_int, "piipp"),
                          "dojo_linesearch_select_dev": (C.c_int, "piippp"), "dojo_linesearch_select": (C.c_int, "piipp")}
LINESEARCH_SYMBOLS = list(_LINESEARCH_SIGNATURES)


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise DojoError("libdojo_hip.so not built (run __graft_entry__.build()); there is no CPU fallback")
        L = C.CDLL(_LIB_PATH)
        for name, (restype, args) in {**_SIGNATURES, **_TRAJOPT_SIGNATURES, **_LIMITS_SIGNATURES, **_CONSTRAINT_SIGNATURES, **_LINESEARCH_SIGNATURES}.items():
            f = getattr(L, name)
            f.restype, f.argtypes = restype, [_KINDS[k] for k in args]
        _lib = L
    return _lib


def addr(x):
    """the address to hand to the library: of a NumPy array, of anything with data_ptr() (a torch tensor); None and a plain int pass through"""
    if x is None or isinstance(x, int):
        return x
    return x.ctypes.data if isinstance(x, np.ndarray) else x.data_ptr()


_p = addr      # the earlier name, kept for callers outside this package that still spell it


def torch_stream(device=None):
    """the handle of torch's current stream on `device`, for the stream argument of the `_dev` entries"""
    import torch
    return torch.cuda.current_stream(device).cuda_stream


class DojoPolicy(C.Structure):
    """include/dojo_hip.h `DojoPolicy`: u_k = U_ff[k] + E (bias + W ((o_k - mean) .* scale)); the members are device pointers for
    dojo_rollout_policy_dev and host pointers for dojo_rollout_policy"""
    _fields_ = [("W", C.c_void_p), ("bias", C.c_void_p), ("mean", C.c_void_p), ("scale", C.c_void_p), ("U_ff", C.c_void_p),
                ("per_env", C.c_int32), ("act_off", C.c_int32), ("na", C.c_int32), ("contact_forces", C.c_int32), ("contact_init", C.c_int32),
                ("reserved", C.c_int32)]


class DojoPolicyAdjoint(C.Structure):
    """include/dojo_hip.h `DojoPolicyAdjoint`: the record, the cotangents and the outputs of dojo_rollout_policy_adjoint_dev (device pointers)"""
    _fields_ = [("DZ", C.c_void_p), ("DU", C.c_void_p), ("OBS", C.c_void_p), ("status", C.c_void_p), ("z0", C.c_void_p), ("Z", C.c_void_p), ("M", C.c_void_p),
                ("G", C.c_void_p), ("G_u", C.c_void_p), ("G_obs", C.c_void_p), ("gW", C.c_void_p), ("gbias", C.c_void_p), ("gU", C.c_void_p), ("gz", C.c_void_p),
                ("cot_space", C.c_int32), ("reserved", C.c_int32)]


class DojoRiccati(C.Structure):
    """include/dojo_hip.h `DojoRiccati`: the record (A, Bm, status), the quadratic cost, the regularisation and the outputs of the Riccati backward pass;
    device pointers for dojo_riccati_dev, host pointers for dojo_riccati"""
    _fields_ = [("A", C.c_void_p), ("Bm", C.c_void_p), ("status", C.c_void_p), ("lx", C.c_void_p), ("lu", C.c_void_p), ("lxx", C.c_void_p), ("luu", C.c_void_p),
                ("lux", C.c_void_p), ("mu", C.c_void_p), ("K", C.c_void_p), ("kff", C.c_void_p), ("fail", C.c_void_p), ("dV", C.c_void_p), ("Vx", C.c_void_p),
                ("Vxx", C.c_void_p), ("act_off", C.c_int32), ("na", C.c_int32)]


class DojoTracking(C.Structure):
    """include/dojo_hip_trajopt.h `DojoTracking`: the inputs (x0, the reference Ubar / Xbar, the gains K / kff, the step lengths alpha) and the outputs (X, U_out, status
    and -- both or neither -- the Jacobians A, Bm) of a rollout in minimal coordinates; device pointers for dojo_rollout_minimal_dev, host pointers for dojo_rollout_minimal"""
    _fields_ = [("x0", C.c_void_p), ("Ubar", C.c_void_p), ("Xbar", C.c_void_p), ("K", C.c_void_p), ("kff", C.c_void_p), ("alpha", C.c_void_p),
                ("X", C.c_void_p), ("U_out", C.c_void_p), ("status", C.c_void_p), ("A", C.c_void_p), ("Bm", C.c_void_p), ("act_off", C.c_int32), ("na", C.c_int32)]


class DojoControlLimits(C.Structure):
    """include/dojo_hip_limits.h `DojoControlLimits`: the limits lo, hi [B][na] of the driven inputs (either may be NULL: none on that side); device pointers
    for the _dev entries, host pointers for dojo_riccati_box and dojo_rollout_minimal_box"""
    _fields_ = [("lo", C.c_void_p), ("hi", C.c_void_p)]


class DojoStageConstraints(C.Structure):
    """include/dojo_hip_constraints.h `DojoStageConstraints`: the linearized constraints of every stage -- Cx [H+1][B][nc][n] and Cu [H][B][nc][na] ([nc][n] and
    [nc][na] when shared; Cu may be NULL: zeros), the row weights w and the multiplier estimates y, [H+1][B][nc] each; device pointers for dojo_riccati_al_dev,
    host pointers for dojo_riccati_al"""
    _fields_ = [("Cx", C.c_void_p), ("Cu", C.c_void_p), ("w", C.c_void_p), ("y", C.c_void_p), ("nc", C.c_int32), ("shared", C.c_int32)]


class DojoQuadraticCost(C.Structure):
    """include/dojo_hip_linesearch.h `DojoQuadraticCost`: Q [n][n], R [na][na], Qf [n][n], goal [n] ([P][n] with goal_per_problem) in the handle dtype; device
    pointers for dojo_linesearch_select_dev, host pointers for dojo_linesearch_select"""
    _fields_ = [("Q", C.c_void_p), ("R", C.c_void_p), ("Qf", C.c_void_p), ("goal", C.c_void_p), ("goal_per_problem", C.c_int32)]


class DojoLineSearch(C.Structure):
    """include/dojo_hip_linesearch.h `DojoLineSearch`: the T trials of P problems (X, U, status, alpha), the model dV, the flags ok, the trajectory the pass was
    taken around (Xcur, Ucur, its cost J0), the costs (J_trial: an output with a cost, an input without; J_cur, J_acc) and the selection (choice, alpha_acc,
    X_new, U_new); device pointers for dojo_linesearch_select_dev, host pointers for dojo_linesearch_select"""
    _fields_ = [("X", C.c_void_p), ("U", C.c_void_p), ("status", C.c_void_p), ("alpha", C.c_void_p), ("dV", C.c_void_p), ("ok", C.c_void_p),
                ("Xcur", C.c_void_p), ("Ucur", C.c_void_p), ("J0", C.c_void_p), ("J_trial", C.c_void_p), ("J_cur", C.c_void_p), ("J_acc", C.c_void_p),
                ("choice", C.c_void_p), ("alpha_acc", C.c_void_p), ("X_new", C.c_void_p), ("U_new", C.c_void_p), ("c1", C.c_double),
                ("act_off", C.c_int32), ("na", C.c_int32)]


MLP_MAX_LAYERS = 4      # DOJO_MLP_MAX_LAYERS


class DojoMlpPolicy(C.Structure):
    """include/dojo_hip.h `DojoMlpPolicy`: the tanh network policy h_l = tanh(b_l + W_l h_{l-1}), u = U_ff + E (b_L + W_L h_{L-1}); theta is the flat
    parameter vector of `pack_mlp`; device pointers for dojo_rollout_mlp_dev, host pointers for dojo_rollout_mlp"""
    _fields_ = [("theta", C.c_void_p), ("mean", C.c_void_p), ("scale", C.c_void_p), ("U_ff", C.c_void_p),
                ("per_env", C.c_int32), ("act_off", C.c_int32), ("n_layers", C.c_int32), ("width", C.c_int32 * (MLP_MAX_LAYERS + 1)),
                ("contact_forces", C.c_int32), ("contact_init", C.c_int32), ("reserved", C.c_int32)]


class DojoMlpAdjoint(C.Structure):
    """include/dojo_hip.h `DojoMlpAdjoint`: the record (with the activations ACT), the cotangents and the outputs of dojo_rollout_mlp_adjoint_dev"""
    _fields_ = [("DZ", C.c_void_p), ("DU", C.c_void_p), ("OBS", C.c_void_p), ("ACT", C.c_void_p), ("status", C.c_void_p), ("z0", C.c_void_p), ("Z", C.c_void_p),
                ("M", C.c_void_p), ("G", C.c_void_p), ("G_u", C.c_void_p), ("G_obs", C.c_void_p), ("gtheta", C.c_void_p), ("gU", C.c_void_p), ("gz", C.c_void_p),
                ("cot_space", C.c_int32), ("reserved", C.c_int32)]


def mlp_sizes(widths):
    """-> (P, nh): the entries of theta, P = sum_l n_l (n_{l-1} + 1), and the hidden units n_1 + .. + n_{L-1} of the widths [n_0, .., n_L]"""
    w = [int(n) for n in widths]
    if not 2 <= len(w) <= MLP_MAX_LAYERS + 1 or min(w) < 1:
        raise ValueError("widths must be [n_0, .., n_L] with 1 <= L <= %d and every width >= 1" % MLP_MAX_LAYERS)
    return sum(w[l] * (w[l - 1] + 1) for l in range(1, len(w))), sum(w[1:-1])


def mlp_policy_struct(theta, mean, scale, U_ff, per_env, act_off, widths, contact_forces=0, contact_init=0):
    """a DojoMlpPolicy from addresses (int or None) and the widths"""
    w = [int(n) for n in widths]
    arr = (C.c_int32 * (MLP_MAX_LAYERS + 1))(*(w + [0] * (MLP_MAX_LAYERS + 1 - len(w)))[:MLP_MAX_LAYERS + 1])
    return DojoMlpPolicy(theta, mean, scale, U_ff, int(per_env), int(act_off), len(w) - 1, arr, int(contact_forces), int(contact_init), 0)


def pack_mlp(weights, biases):
    """weights [W_1 .. W_L], W_l [n_l, n_{l-1}] (or [B, n_l, n_{l-1}]: one policy per environment), biases [b_1 .. b_L], b_l [n_l] (or [B, n_l])
    -> (theta, widths): theta [P] (or [B, P]) in the layout of the ABI -- layer after layer W_l row-major, then b_l -- and widths [n_0, .., n_L]"""
    Ws = [np.asarray(W) for W in weights]; bs = [np.asarray(b) for b in biases]
    if not Ws or len(Ws) != len(bs):
        raise ValueError("pack_mlp needs one bias per weight matrix")
    lead = Ws[0].shape[:-2]
    widths = [int(Ws[0].shape[-1])]
    parts = []
    for W, b in zip(Ws, bs):
        if W.ndim != len(lead) + 2 or W.shape[:-2] != lead or W.shape[-1] != widths[-1] or b.shape != lead + (W.shape[-2],):
            raise ValueError("pack_mlp: W_l must be [.., n_l, n_{l-1}] and b_l [.., n_l] with matching widths")
        widths.append(int(W.shape[-2]))
        parts += [W.reshape(lead + (-1,)), b]
    return np.ascontiguousarray(np.concatenate(parts, axis=-1)), widths


def unpack_mlp(theta, widths):
    """the inverse of pack_mlp: theta [P] or [B, P] -> (weights, biases), views into theta"""
    theta = np.asarray(theta); w = [int(n) for n in widths]
    P, _ = mlp_sizes(w)
    if theta.shape[-1] != P:
        raise ValueError("theta has %d entries, the widths %s need %d" % (theta.shape[-1], w, P))
    lead, o = theta.shape[:-1], 0
    Ws, bs = [], []
    for l in range(1, len(w)):
        n = w[l] * w[l - 1]
        Ws.append(theta[..., o:o + n].reshape(lead + (w[l], w[l - 1]))); o += n
        bs.append(theta[..., o:o + w[l]]); o += w[l]
    return Ws, bs


# columns of a Storage row (src/simulation/storage.jl:15-24)
STORAGE_FIELDS = {"x": slice(0, 3), "q": slice(3, 7), "v": slice(7, 10), "w": slice(10, 13), "px": slice(13, 16), "pq": slice(16, 19),
                  "vl": slice(19, 22), "wl": slice(22, 25)}


def device_count():
    return lib().dojo_device_count()


def _chk(rc):
    if rc != 0:
        raise DojoError("libdojo_hip error %d: %s" % (rc, lib().dojo_last_error().decode()))


class BatchedMechanism:
    """B independent copies of one Dojo `Mechanism` resident on one GPU."""

    def __init__(self, spec, batch, dtype="f32", device=0, opts=None):
        self.spec, self.batch = spec, int(batch)
        self.np_dtype = np.float32 if dtype in ("f32", np.float32) else np.float64
        self.dtype_code = 1 if self.np_dtype == np.float32 else 0
        self._topo, self._keep = spec.to_ctypes()
        self.csg_per = 12 if any(c.model == 2 for c in spec.contacts) else 8     # exported [s; γ] scalars per contact (LinearContact: 6 + 6)
        self.h = C.c_void_p()
        _chk(lib().dojo_create(C.byref(self._topo), self.batch, self.dtype_code, int(device), C.byref(self.h)))
        d = CDims()
        _chk(lib().dojo_get_dims(self.h, C.byref(d)))
        self.dims = d
        # (the device exports [s(4); γ(4)] per contact for every contact model: an ImpactContact's entries are [s, 1, 0, 0, γ, 1, 0, 0])
        assert d.nu == spec.nu and d.n_joint_impulses == spec.n_joint_impulses and d.n_solution == spec.n_joint_impulses + 6 * spec.Nb + self.csg_per * len(spec.contacts)
        self.set_options(opts or SolverOptions())

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            lib().dojo_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_options(self, opts):
        self.opts = opts
        o = opts.to_c()
        _chk(lib().dojo_set_options(self.h, C.byref(o)))

    def set_gradient_mode(self, mode):
        _chk(lib().dojo_set_gradient_mode(self.h, int(mode)))

    def set_async(self, on=True):
        """dojo_step_dev no longer joins its environment groups into the caller's stream; join() does it once.  on = 2: pipelined groups as well
        (the IFT kernel of a group's step runs next to the group's next step kernel, include/dojo_hip.h)"""
        _chk(lib().dojo_set_async(self.h, 2 if on == 2 else int(bool(on))))

    def set_groups(self, n):
        _chk(lib().dojo_set_groups(self.h, int(n)))

    def set_iteration_cap(self, cap):
        """dojo_set_iteration_cap: solves unfinished after `cap` Newton iterations go on in the continuation kernel (line-search trials
        side by side) in steps that are joined into the caller's stream; 0 / < 0: off (the default).  Include/dojo_hip.h has the measurements."""
        _chk(lib().dojo_set_iteration_cap(self.h, int(cap)))

    def set_dispatch_order(self, mode):
        """dojo_set_dispatch_order: 0 batch order, 1 (default) the previous step's longest solves first where a joined step has more workgroups
        than the GPU holds at once, 2 always.  Results do not depend on it."""
        _chk(lib().dojo_set_dispatch_order(self.h, int(mode)))

    def join(self, stream=None):
        _chk(lib().dojo_join(self.h, stream or 0))

    # ---- multi-GPU: RCCL communicator of the handle (one process per GPU) ----
    @staticmethod
    def comm_unique_id():
        buf = (C.c_char * 128)()
        _chk(lib().dojo_comm_unique_id(buf))
        return bytes(buf)

    def comm_init(self, rank, world, unique_id):
        _chk(lib().dojo_comm_init(self.h, int(rank), int(world), unique_id))

    def allgather_dev(self, send_ptr, recv_ptr, count, as_int32=False, stream=None):
        _chk(lib().dojo_allgather_dev(self.h, send_ptr, recv_ptr, int(count), int(bool(as_int32)), stream or 0))

    def set_refinement(self, stiffness):
        """Refine the linear solves of environments whose cones reach max gamma/s > stiffness (inf: never, 0: always)."""
        _chk(lib().dojo_set_refinement(self.h, float(stiffness)))

    def _arr(self, a, shape):
        a = np.ascontiguousarray(a, dtype=self.np_dtype)
        if a.shape != shape:
            raise ValueError("expected shape %s, got %s" % (shape, a.shape))
        return a

    def _controls(self, U, steps):
        """-> (U, H) of an open-loop rollout: the horizon is U's, or `steps` without controls"""
        if U is not None and self.spec.nu:
            U = np.ascontiguousarray(U, dtype=self.np_dtype); H = U.shape[0]
            assert U.shape == (H, self.batch, self.spec.nu)
            return U, H
        return None, int(steps)

    @staticmethod
    def _space(name, value):
        """cot_space / tan_space -> 0 (tangent coordinates) or 1 (state coordinates)"""
        if value not in ("tangent", "state", 0, 1):
            raise ValueError("%s must be 'tangent' or 'state'" % name)
        return 1 if value in ("state", 1) else 0

    def _cotangents(self, who, G, steps, cot_space):
        """-> (G, H, cs): the cotangents in the handle dtype, the horizon they hold and the code of cot_space"""
        B, s = self.batch, self.spec
        cs = self._space("cot_space", cot_space)
        if G is None:
            raise ValueError("%s needs the cotangents G of the loss w.r.t. the state after every step" % who)
        G = np.ascontiguousarray(G, dtype=self.np_dtype); H = G.shape[0]
        if G.shape != (H, B, s.nz if cs else s.nx):
            raise ValueError("expected G of shape %s, got %s" % ((H, B, s.nz if cs else s.nx), G.shape))
        if steps is not None and int(steps) != H:
            raise ValueError("steps = %d but G holds %d steps" % (int(steps), H))
        return G, H, cs

    def _policy_terms(self, mean, scale, U_ff, H, nobs):
        """the optional arguments both policies share, checked in this order: mean, scale [nobs], U_ff [H,B,nu]"""
        return (None if mean is None else self._arr(mean, (nobs,)), None if scale is None else self._arr(scale, (nobs,)),
                None if U_ff is None else self._arr(U_ff, (H, self.batch, self.spec.nu)))

    def _affine_policy(self, W, bias, mean, scale, U_ff, H, nobs, act_off, contact_forces=False, contact_init=0):
        """-> (DojoPolicy, the arrays it points to: W, bias, mean, scale, U_ff in the handle dtype)"""
        W = np.ascontiguousarray(W, dtype=self.np_dtype)
        if W.ndim not in (2, 3):
            raise ValueError("W must be [na, nobs] or [B, na, nobs]")
        per_env, na = W.ndim == 3, W.shape[-2]
        W = self._arr(W, (self.batch, na, nobs) if per_env else (na, nobs))
        bias = None if bias is None else self._arr(bias, (self.batch, na) if per_env else (na,))
        arrays = (W, bias) + self._policy_terms(mean, scale, U_ff, H, nobs)
        return DojoPolicy(*map(addr, arrays), int(per_env), int(act_off), int(na), int(bool(contact_forces)), int(contact_init), 0), arrays

    def _mlp_policy(self, theta, widths, mean, scale, U_ff, H, nobs, act_off, contact_forces=False, contact_init=0):
        """-> (DojoMlpPolicy, the arrays it points to: theta, mean, scale, U_ff in the handle dtype)"""
        theta, w, per_env = self._mlp_args(theta, widths)
        arrays = (theta,) + self._policy_terms(mean, scale, U_ff, H, nobs)
        return mlp_policy_struct(*map(addr, arrays), per_env, act_off, w, bool(contact_forces), contact_init), arrays

    def _closed_loop_outputs(self, H, nobs):
        """-> Z [H,B,13Nb], OBS [H+1,B,nobs], U [H,B,nu], status [H,B]"""
        B, s, H = self.batch, self.spec, max(H, 0)
        return (np.empty((H, B, s.nz), self.np_dtype), np.empty((H + 1, B, nobs), self.np_dtype), np.empty((H, B, s.nu), self.np_dtype),
                np.empty((H, B), np.int32))

    def step(self, z, u=None, with_gradient=False):
        B, s = self.batch, self.spec
        z = self._arr(z, (B, s.nz))
        u = None if (u is None or s.nu == 0) else self._arr(u, (B, s.nu))
        zn = np.empty_like(z); st = np.empty(B, np.int32); it = np.empty(B, np.int32)
        _chk(lib().dojo_step(self.h, addr(z), addr(u), addr(zn), addr(st), addr(it), int(with_gradient)))
        return zn, st, it

    def step_impulses(self, z, jf):
        """The mehrotra!(mechanism) seam: one step with the controls already folded into the bodies' impulses,
        jf [B, Nb, 6] = [state.JF2 (world); state.Jtau2 (body frame)] (src/integrators/constraint.jl:20-21)."""
        B, s = self.batch, self.spec
        z = self._arr(z, (B, s.nz))
        jf = self._arr(np.asarray(jf).reshape(B, 6 * s.Nb), (B, 6 * s.Nb))
        zn = np.empty_like(z); st = np.empty(B, np.int32); it = np.empty(B, np.int32)
        _chk(lib().dojo_step_impulses(self.h, addr(z), addr(jf), addr(zn), addr(st), addr(it)))
        return zn, st, it

    def next_state(self, z):
        """get_next_state of a state whose velocities are its solution: maps dojo_step's return (the internal state after
        update_state!) to the vector the reference's step! literally returns."""
        z = self._arr(z, (self.batch, self.spec.nz)); zo = np.empty_like(z)
        _chk(lib().dojo_next_state(self.h, addr(z), addr(zo)))
        return zo

    def diagnostics(self, read=True):
        """[B, 2]: max gamma/s of the cones and the largest Gauss-Jordan multiplier at the last step's final linearization
        (the first call switches the recording on)"""
        dg = np.zeros((self.batch, 2)) if read else None
        _chk(lib().dojo_get_diagnostics(self.h, addr(dg)))
        return dg

    def get_mu(self):
        mu = np.empty(self.batch, np.float64)
        _chk(lib().dojo_get_mu(self.h, addr(mu)))
        return mu

    def kernel_build(self):
        """dojo_get_kernel_build: (family, MAXC, waves) of the kernel build that steps this handle -- family one of KERNEL_FAMILIES,
        waves 1 / 2 = the quad mapping's wavefronts per workgroup, 0 = the lane mapping"""
        out = np.zeros(3, np.int32)
        _chk(lib().dojo_get_kernel_build(self.h, addr(out)))
        return KERNEL_FAMILIES[int(out[0])], int(out[1]), int(out[2])

    def last_error(self):
        return lib().dojo_handle_error(self.h).decode()

    def get_solution(self):
        B, s = self.batch, self.spec
        vel = np.empty((B, 6 * s.Nb), self.np_dtype)
        ji = np.empty((B, max(s.n_joint_impulses, 1)), self.np_dtype)
        cs = np.empty((B, max(self.csg_per * len(s.contacts), 1)), self.np_dtype)
        _chk(lib().dojo_get_solution(self.h, addr(vel), addr(ji), addr(cs)))
        return vel, ji[:, :s.n_joint_impulses], cs[:, :self.csg_per * len(s.contacts)]

    def gradients(self):
        B, s = self.batch, self.spec
        dz = np.empty((B, s.nx, s.nx), self.np_dtype)
        du = np.empty((B, s.nx, max(s.nu, 1)), self.np_dtype)
        _chk(lib().dojo_gradients(self.h, addr(dz), addr(du)))
        return dz, du[:, :, :s.nu]

    def rollout(self, z0, U=None, steps=None, record=True):
        B, s = self.batch, self.spec
        z0 = self._arr(z0, (B, s.nz))
        U, H = self._controls(U, steps)
        Z = np.empty((H, B, s.nz), self.np_dtype) if record else None
        st = np.empty((H, B), np.int32)
        _chk(lib().dojo_rollout(self.h, addr(z0), addr(U), H, addr(Z), addr(st)))
        return Z, st

    def rollout_gradients(self, z0, U=None, G=None, steps=None, cot_space="tangent"):
        """Reverse-mode rollout (dojo_rollout_gradients): the rollout of `rollout`, and the gradient of a trajectory loss w.r.t. the controls
        and the initial state from the recorded IFT Jacobians, which stay on the device.  G [H,B,nx] (cot_space "tangent": the cotangent of
        the loss w.r.t. the state after every step in the coordinates of dz, [x; v; phi; omega] per body) or [H,B,13Nb] ("state": w.r.t.
        the state vector itself).  Returns (Z [H,B,13Nb], status [H,B], gU [H,B,nu], gz0 [B,nx] in tangent coordinates); nothing flows
        through a failed step.  GRAD_CONSISTENT (set_gradient_mode) is the mode whose chain is the derivative of the rollout."""
        B, s = self.batch, self.spec
        z0 = self._arr(z0, (B, s.nz))
        G, H, cs = self._cotangents("rollout_gradients", G, steps, cot_space)
        U = self._arr(U, (H, B, s.nu)) if (U is not None and s.nu) else None
        Z = np.empty((H, B, s.nz), self.np_dtype); st = np.empty((H, B), np.int32)
        gU = np.zeros((H, B, s.nu), self.np_dtype); gz = np.empty((B, s.nx), self.np_dtype)
        _chk(lib().dojo_rollout_gradients(self.h, addr(z0), addr(U), H, addr(G), cs, addr(Z), addr(st), addr(gU) if s.nu else None, addr(gz)))
        return Z, st, gU, gz

    def set_contact_data(self, theta):
        """set_data!(mechanism.contacts, theta) on the live handle (dojo_set_contact_data): theta [Nc, 5] = [friction_coefficient, contact_radius,
        contact_origin(3)] per contact, shared by all environments.  The handle then steps as one created with theta; `contact_gradients` needs a new
        differentiable step first."""
        Nc = len(self.spec.contacts)
        th = np.ascontiguousarray(np.asarray(theta, dtype=np.float64).reshape(Nc, 5))
        _chk(lib().dojo_set_contact_data(self.h, addr(th) if Nc else None))

    def contact_data(self):
        """the handle's contact data [Nc, 5] (dojo_get_contact_data)"""
        th = np.zeros((len(self.spec.contacts), 5), np.float64)
        _chk(lib().dojo_get_contact_data(self.h, addr(th) if len(th) else None))
        return th

    def rollout_data_gradients(self, z0, U=None, G=None, steps=None, cot_space="tangent", per_env=False):
        """Reverse-mode rollout w.r.t. the contact data (dojo_rollout_data_gradients): the rollout of `rollout`, and the gradient of a trajectory loss
        w.r.t. theta = `contact_data()`, the controls and the initial state, from the recorded IFT Jacobians of every step (state, control and
        contact-data columns), which stay on the device.  G and cot_space as in `rollout_gradients`.  Returns (Z [H,B,13Nb], status [H,B],
        gtheta [Nc,5] summed over the batch, gtheta_env [B,Nc,5] (per_env=True, else None), gU [H,B,nu], gz0 [B,nx] tangent)."""
        B, s = self.batch, self.spec
        Nc = len(s.contacts)
        z0 = self._arr(z0, (B, s.nz))
        G, H, cs = self._cotangents("rollout_data_gradients", G, steps, cot_space)
        U = self._arr(U, (H, B, s.nu)) if (U is not None and s.nu) else None
        Z = np.empty((H, B, s.nz), self.np_dtype); st = np.empty((H, B), np.int32)
        gth = np.zeros((Nc, 5), self.np_dtype); gte = np.zeros((B, Nc, 5), self.np_dtype) if per_env else None
        gU = np.zeros((H, B, s.nu), self.np_dtype); gz = np.empty((B, s.nx), self.np_dtype)
        _chk(lib().dojo_rollout_data_gradients(self.h, addr(z0), addr(U), H, addr(G), cs, addr(Z), addr(st), addr(gth) if Nc else None,
                                               addr(gte) if (per_env and Nc) else None, addr(gU) if s.nu else None, addr(gz)))
        return Z, st, gth, gte, gU, gz

    def rollout_tangents(self, z0, U=None, dz0=None, dU=None, dtheta=None, steps=None, tan_space="tangent"):
        """Forward-mode rollout (dojo_rollout_tangents): the rollout of `rollout`, and T tangent directions pushed through the recorded IFT Jacobians of
        every step in one pass over the record, which stays on the device.  dz0 [B,T,nx] (tangent coordinates [x; v; phi; omega] per body), dU [H,B,T,nu],
        dtheta [T,Nc,5] or [T,5Nc] (directions of `contact_data()`, shared by the batch); each may be None (= zeros), not all three; T is taken from
        whichever is given.  Returns (Z [H,B,13Nb], status [H,B], dZ [H,B,T,nx] -- or [H,B,T,13Nb] with tan_space "state": the tangent of the state
        vector itself, dq = q (x) (0, phi)).  Nothing flows through a failed step: the tangent of the state after it is 0."""
        B, s = self.batch, self.spec
        nth = 5 * len(s.contacts)
        z0 = self._arr(z0, (B, s.nz))
        ts = self._space("tan_space", tan_space)
        dz0 = None if dz0 is None else np.ascontiguousarray(dz0, dtype=self.np_dtype)
        dU = None if (dU is None or not s.nu) else np.ascontiguousarray(dU, dtype=self.np_dtype)
        dtheta = None if (dtheta is None or not nth) else np.ascontiguousarray(dtheta, dtype=self.np_dtype)
        if dtheta is not None:
            dtheta = dtheta.reshape(dtheta.shape[0], -1)
        Ts = [a.shape[i] for a, i in ((dz0, 1), (dU, 2), (dtheta, 0)) if a is not None and a.ndim > i]
        if not Ts:
            raise ValueError("rollout_tangents needs at least one of dz0, dU, dtheta (dU counts only with nu > 0, dtheta only with contacts)")
        T = int(Ts[0])
        if any(int(t) != T for t in Ts):
            raise ValueError("dz0, dU and dtheta hold different numbers of tangents: %s" % Ts)
        Hs = [np.shape(a)[0] for a in (U if s.nu else None, dU) if a is not None] + ([int(steps)] if steps is not None else [])
        if not Hs:
            raise ValueError("rollout_tangents needs the horizon: U, dU or steps")
        H = int(Hs[0])
        if any(int(h) != H for h in Hs):
            raise ValueError("U, dU and steps disagree about the horizon: %s" % Hs)
        U = self._arr(U, (H, B, s.nu)) if (U is not None and s.nu) else None
        for name, a, shape in (("dz0", dz0, (B, T, s.nx)), ("dU", dU, (H, B, T, s.nu)), ("dtheta", dtheta, (T, nth))):
            if a is not None and a.shape != shape:
                raise ValueError("expected %s of shape %s, got %s" % (name, shape, a.shape))
        Z = np.empty((H, B, s.nz), self.np_dtype); st = np.empty((H, B), np.int32)
        dZ = np.empty((H, B, T, s.nz if ts else s.nx), self.np_dtype)
        _chk(lib().dojo_rollout_tangents(self.h, addr(z0), addr(U), H, T, addr(dz0), addr(dU), addr(dtheta), ts, addr(Z), addr(st), addr(dZ)))
        return Z, st, dZ

    def riccati(self, A, Bm, lx, lu, lxx, luu, lux=None, mu=None, status=None, act_off=0, na=None, value=True):
        """dojo_riccati (host arrays): the backward pass of iLQR in minimal coordinates over the Jacobians A [H,B,n,n], Bm [H,B,n,nu] of H steps (minimal_gradients'
        jx, ju), n = 2 nu, for the quadratic cost lx [H+1,B,n], lu [H,B,na], lxx [H+1,B,n,n], luu [H,B,na,na], lux [H,B,na,n] (None: zeros), the regularisation
        mu [B] (None: zeros) and the step status [H,B] (None: all solved).  -> K [H,B,na,n], kff [H,B,na], dV [B,2], fail [B] (0, or 1 + the step whose Cholesky
        failed) and, with value, Vx [B,n], Vxx [B,n,n]."""
        B, nu = self.batch, self.spec.nu; n = 2 * nu
        H = int(np.shape(A)[0]); na = int(nu - act_off if na is None else na)
        A = self._arr(A, (H, B, n, n)); Bm = self._arr(Bm, (H, B, n, nu))
        lx = self._arr(lx, (H + 1, B, n)); lu = self._arr(lu, (H, B, na)); lxx = self._arr(lxx, (H + 1, B, n, n)); luu = self._arr(luu, (H, B, na, na))
        lux = None if lux is None else self._arr(lux, (H, B, na, n)); mu = None if mu is None else self._arr(mu, (B,))
        status = None if status is None else np.ascontiguousarray(status, dtype=np.int32)
        K = np.empty((H, B, na, n), self.np_dtype); kff = np.empty((H, B, na), self.np_dtype); fail = np.empty(B, np.int32); dV = np.empty((B, 2), self.np_dtype)
        Vx = np.empty((B, n), self.np_dtype) if value else None; Vxx = np.empty((B, n, n), self.np_dtype) if value else None
        r = DojoRiccati(*map(addr, (A, Bm, status, lx, lu, lxx, luu, lux, mu, K, kff, fail, dV, Vx, Vxx)), int(act_off), na)
        _chk(lib().dojo_riccati(self.h, H, C.byref(r)))
        return (K, kff, dV, fail, Vx, Vxx) if value else (K, kff, dV, fail)

    def rollout_minimal(self, x0, steps=None, Ubar=None, Xbar=None, K=None, kff=None, alpha=None, act_off=0, na=None, jacobians=False):
        """dojo_rollout_minimal (host arrays): H steps in minimal coordinates from x0 [B,n], n = 2 nu, under the tracking controller
        u_k = Ubar[k] + E (alpha kff[k] + K[k] (x_k - Xbar[k])) evaluated on the device between the steps.  Ubar [H,B,nu], Xbar [H+1,B,n], K [H,B,na,n], kff [H,B,na]
        (the outputs of `riccati`), alpha [B]; each may be None (zeros; alpha: ones).  The horizon is that of Ubar, K or kff, or `steps`.  The controller drives the
        inputs act_off .. act_off + na - 1 (na = nu - act_off by default).  -> (X [H+1,B,n], U [H,B,nu], status [H,B]) and, with jacobians, A [H,B,n,n], Bm [H,B,n,nu]:
        `minimal_gradients`' jx, ju of every step, in the handle's gradient mode."""
        B, nu = self.batch, self.spec.nu; n = 2 * nu
        na = int(nu - act_off if na is None else na)
        Hs = [np.shape(a)[0] for a in (Ubar, K, kff) if a is not None] + ([int(steps)] if steps is not None else [])
        if not Hs:
            raise ValueError("rollout_minimal needs the horizon: Ubar, K, kff or steps")
        H = int(Hs[0])
        if any(int(h) != H for h in Hs):
            raise ValueError("Ubar, K, kff and steps disagree about the horizon: %s" % Hs)
        opt = lambda a, shape: None if a is None else self._arr(a, shape)
        ins = (self._arr(x0, (B, n)), opt(Ubar, (H, B, nu)), opt(Xbar, (H + 1, B, n)), opt(K, (H, B, na, n)), opt(kff, (H, B, na)), opt(alpha, (B,)))
        X = np.empty((H + 1, B, n), self.np_dtype); U = np.empty((H, B, nu), self.np_dtype); st = np.empty((H, B), np.int32)
        A = np.empty((H, B, n, n), self.np_dtype) if jacobians else None; Bm = np.empty((H, B, n, nu), self.np_dtype) if jacobians else None
        t = DojoTracking(*map(addr, ins + (X, U, st, A, Bm)), int(act_off), na)
        _chk(lib().dojo_rollout_minimal(self.h, H, C.byref(t)))
        return (X, U, st, A, Bm) if jacobians else (X, U, st)

    def _limits(self, lo, hi, na):
        """lo, hi: None, a scalar, [na] or [B, na] -> the two [B, na] arrays (None stays None) and the DojoControlLimits over them"""
        arrs = [None if a is None else np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=self.np_dtype), (self.batch, na))) for a in (lo, hi)]
        return arrs, DojoControlLimits(addr(arrs[0]), addr(arrs[1]))

    def riccati_box(self, A, Bm, lx, lu, lxx, luu, U, lo=None, hi=None, lux=None, mu=None, status=None, act_off=0, na=None, value=True):
        """dojo_riccati_box (host arrays): `riccati` under the control limits lo <= U[k][act] + kff[k] <= hi (control-limited DDP: a box QP per step, the gain
        rows of clamped inputs are zero).  U [H,B,nu]: the controls the pass is taken around; lo, hi: None, a scalar, [na] or [B,na], +-inf allowed.
        -> K, kff, dV, fail (0; 1 + k: the Cholesky of step k failed; -(1 + k): the QP of step k failed or its box is empty), active [H,B] int64 (bit i: input
        act_off + i clamped), qp_iters [H,B] and, with value, Vx, Vxx."""
        B, nu = self.batch, self.spec.nu; n = 2 * nu
        H = int(np.shape(A)[0]); na = int(nu - act_off if na is None else na)
        A = self._arr(A, (H, B, n, n)); Bm = self._arr(Bm, (H, B, n, nu)); U = self._arr(U, (H, B, nu))
        lx = self._arr(lx, (H + 1, B, n)); lu = self._arr(lu, (H, B, na)); lxx = self._arr(lxx, (H + 1, B, n, n)); luu = self._arr(luu, (H, B, na, na))
        lux = None if lux is None else self._arr(lux, (H, B, na, n)); mu = None if mu is None else self._arr(mu, (B,))
        status = None if status is None else np.ascontiguousarray(status, dtype=np.int32)
        K = np.empty((H, B, na, n), self.np_dtype); kff = np.empty((H, B, na), self.np_dtype); fail = np.empty(B, np.int32); dV = np.empty((B, 2), self.np_dtype)
        Vx = np.empty((B, n), self.np_dtype) if value else None; Vxx = np.empty((B, n, n), self.np_dtype) if value else None
        active = np.empty((H, B), np.int64); qp_iters = np.empty((H, B), np.int32)
        keep, lim = self._limits(lo, hi, na)
        r = DojoRiccati(*map(addr, (A, Bm, status, lx, lu, lxx, luu, lux, mu, K, kff, fail, dV, Vx, Vxx)), int(act_off), na)
        _chk(lib().dojo_riccati_box(self.h, H, C.byref(r), C.byref(lim), addr(U), addr(active), addr(qp_iters)))
        return (K, kff, dV, fail, active, qp_iters, Vx, Vxx) if value else (K, kff, dV, fail, active, qp_iters)

    def riccati_al(self, A, Bm, lx, lu, lxx, luu, Cx, w, y, Cu=None, shared=False, U=None, lo=None, hi=None, lux=None, mu=None, status=None, act_off=0, na=None,
                   value=True):
        """dojo_riccati_al (host arrays): `riccati_box` with the augmented-Lagrangian terms of nc linearized constraint rows per stage added to the step's
        model inside the kernel: G' diag(w) G to the Hessian and G' y to the gradient, G = [Cx Cu].  Cx [H+1,B,nc,n], Cu [H,B,nc,na] or None (zeros) -- [nc,n]
        and [nc,na] with shared --, w, y [H+1,B,nc] (a row with w = y = 0 is not read).  lo, hi as in riccati_box; both None: no limits, and U may be None.
        nc = 0: Cx, w, y may be None.  -> what riccati_box returns."""
        B, nu = self.batch, self.spec.nu; n = 2 * nu
        H = int(np.shape(A)[0]); na = int(nu - act_off if na is None else na)
        nc = 0 if w is None else int(np.shape(w)[-1])
        A = self._arr(A, (H, B, n, n)); Bm = self._arr(Bm, (H, B, n, nu)); U = None if U is None else self._arr(U, (H, B, nu))
        lx = self._arr(lx, (H + 1, B, n)); lu = self._arr(lu, (H, B, na)); lxx = self._arr(lxx, (H + 1, B, n, n)); luu = self._arr(luu, (H, B, na, na))
        lux = None if lux is None else self._arr(lux, (H, B, na, n)); mu = None if mu is None else self._arr(mu, (B,))
        status = None if status is None else np.ascontiguousarray(status, dtype=np.int32)
        opt = lambda a, shape: None if a is None else self._arr(a, shape)
        Cx = opt(Cx, (nc, n) if shared else (H + 1, B, nc, n)); Cu = opt(Cu, (nc, na) if shared else (H, B, nc, na))
        w = opt(w, (H + 1, B, nc)); y = opt(y, (H + 1, B, nc))
        K = np.empty((H, B, na, n), self.np_dtype); kff = np.empty((H, B, na), self.np_dtype); fail = np.empty(B, np.int32); dV = np.empty((B, 2), self.np_dtype)
        Vx = np.empty((B, n), self.np_dtype) if value else None; Vxx = np.empty((B, n, n), self.np_dtype) if value else None
        active = np.empty((H, B), np.int64); qp_iters = np.empty((H, B), np.int32)
        keep, lim = self._limits(lo, hi, na)
        con = DojoStageConstraints(addr(Cx), addr(Cu), addr(w), addr(y), nc, int(bool(shared)))
        r = DojoRiccati(*map(addr, (A, Bm, status, lx, lu, lxx, luu, lux, mu, K, kff, fail, dV, Vx, Vxx)), int(act_off), na)
        _chk(lib().dojo_riccati_al(self.h, H, C.byref(r), None if lo is None and hi is None else C.byref(lim), addr(U), C.byref(con), addr(active), addr(qp_iters)))
        return (K, kff, dV, fail, active, qp_iters, Vx, Vxx) if value else (K, kff, dV, fail, active, qp_iters)

    def rollout_minimal_box(self, x0, lo=None, hi=None, steps=None, Ubar=None, Xbar=None, K=None, kff=None, alpha=None, act_off=0, na=None, jacobians=False):
        """dojo_rollout_minimal_box (host arrays): `rollout_minimal` with the driven inputs clamped into [lo, hi] (None, a scalar, [na] or [B,na]) before they are
        rounded and stepped -> what `rollout_minimal` returns."""
        B, nu = self.batch, self.spec.nu; n = 2 * nu
        na = int(nu - act_off if na is None else na)
        Hs = [np.shape(a)[0] for a in (Ubar, K, kff) if a is not None] + ([int(steps)] if steps is not None else [])
        if not Hs:
            raise ValueError("rollout_minimal_box needs the horizon: Ubar, K, kff or steps")
        H = int(Hs[0])
        if any(int(h) != H for h in Hs):
            raise ValueError("Ubar, K, kff and steps disagree about the horizon: %s" % Hs)
        opt = lambda a, shape: None if a is None else self._arr(a, shape)
        ins = (self._arr(x0, (B, n)), opt(Ubar, (H, B, nu)), opt(Xbar, (H + 1, B, n)), opt(K, (H, B, na, n)), opt(kff, (H, B, na)), opt(alpha, (B,)))
        X = np.empty((H + 1, B, n), self.np_dtype); U = np.empty((H, B, nu), self.np_dtype); st = np.empty((H, B), np.int32)
        A = np.empty((H, B, n, n), self.np_dtype) if jacobians else None; Bm = np.empty((H, B, n, nu), self.np_dtype) if jacobians else None
        keep, lim = self._limits(lo, hi, na)
        t = DojoTracking(*map(addr, ins + (X, U, st, A, Bm)), int(act_off), na)
        _chk(lib().dojo_rollout_minimal_box(self.h, H, C.byref(t), C.byref(lim)))
        return (X, U, st, A, Bm) if jacobians else (X, U, st)

    def rollout_minimal_fan(self, T, x0, lo=None, hi=None, steps=None, Ubar=None, Xbar=None, K=None, kff=None, alpha=None, act_off=0, na=None):
        """dojo_rollout_minimal_fan (host arrays): T trials of P = batch / T problems in one rollout.  x0 [P,n], Ubar [H,P,nu], Xbar [H+1,P,n], K [H,P,na,n],
        kff [H,P,na], lo / hi (None, a scalar, [na] or [P,na]) are per problem; alpha [T,P] is per environment (e = tr P + p).  lo and hi both None: no limits.
        -> X [H+1,T P,n], U [H,T P,nu], status [H,T P]: what `rollout_minimal_box` (`rollout_minimal` without limits) gives with the inputs repeated T times."""
        B, nu, T = self.batch, self.spec.nu, int(T); n = 2 * nu
        P = B // T if T >= 1 and B % T == 0 else B          # (a T the library refuses: the arrays' shapes are then not looked at here)
        na = int(nu - act_off if na is None else na)
        Hs = [np.shape(a)[0] for a in (Ubar, K, kff) if a is not None] + ([int(steps)] if steps is not None else [])
        if not Hs:
            raise ValueError("rollout_minimal_fan needs the horizon: Ubar, K, kff or steps")
        H = int(Hs[0])
        if any(int(h) != H for h in Hs):
            raise ValueError("Ubar, K, kff and steps disagree about the horizon: %s" % Hs)
        opt = lambda a, shape: None if a is None else self._arr(a, shape)
        ins = (self._arr(x0, (P, n)), opt(Ubar, (H, P, nu)), opt(Xbar, (H + 1, P, n)), opt(K, (H, P, na, n)), opt(kff, (H, P, na)), opt(alpha, (B // P, P)))
        X = np.empty((H + 1, B, n), self.np_dtype); U = np.empty((H, B, nu), self.np_dtype); st = np.empty((H, B), np.int32)
        lims = [None if a is None else np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=self.np_dtype), (P, na))) for a in (lo, hi)]
        lim = DojoControlLimits(addr(lims[0]), addr(lims[1]))
        t = DojoTracking(*map(addr, ins + (X, U, st, None, None)), int(act_off), na)
        _chk(lib().dojo_rollout_minimal_fan(self.h, H, T, C.byref(t), None if lo is None and hi is None else C.byref(lim)))
        return X, U, st

    def linesearch_select(self, T, X, U, alpha, dV, Xcur, Ucur, cost=None, status=None, ok=None, J0=None, J_trial=None, c1=1e-4, act_off=0, na=None, gather=True):
        """dojo_linesearch_select (host arrays) on the T trials X [H+1,T P,n], U [H,T P,nu], status [H,T P] of a fan: the first trial tr of every problem with
        ok != 0, no failed step and J_tr <= J0 + c1 (a dV[0] + a^2 dV[1]), a = alpha[tr, p].  cost = (Q, R, Qf, goal) (goal [n] or [P,n]): the costs are computed on
        the device in fp64 (J0 from Xcur, Ucur unless given); cost None: J_trial [T,P] and J0 [P] are the caller's.
        -> dict: choice [P] int32 (-1: none), alpha [P], J_trial [T,P], J_cur [P], J_acc [P] (float64) and, with gather, X [H+1,P,n], U [H,P,nu]: the accepted
        trial's columns, or Xcur / Ucur."""
        B, nu, T = self.batch, self.spec.nu, int(T); n = 2 * nu
        P = B // T if T >= 1 and B % T == 0 else B
        na = int(nu - act_off if na is None else na)
        H = int(np.shape(U)[0])
        X = self._arr(X, (H + 1, B, n)); U = self._arr(U, (H, B, nu)); alpha = self._arr(alpha, (B // P, P)); dV = self._arr(dV, (P, 2))
        Xcur = self._arr(Xcur, (H + 1, P, n)); Ucur = self._arr(Ucur, (H, P, nu))
        status = None if status is None else np.ascontiguousarray(status, dtype=np.int32); ok = None if ok is None else np.ascontiguousarray(ok, dtype=np.int32)
        J0 = None if J0 is None else np.ascontiguousarray(J0, dtype=np.float64)
        J_trial = np.empty((B // P, P), np.float64) if cost is not None else None if J_trial is None else np.array(J_trial, dtype=np.float64, order="C")
        J_cur = np.empty(P, np.float64); J_acc = np.empty(P, np.float64); choice = np.empty(P, np.int32); a_acc = np.empty(P, self.np_dtype)
        Xn = np.empty((H + 1, P, n), self.np_dtype) if gather else None; Un = np.empty((H, P, nu), self.np_dtype) if gather else None
        qc = None
        if cost is not None:
            Q, R, Qf, goal = cost
            per = np.ndim(goal) == 2
            keep = (self._arr(Q, (n, n)), self._arr(R, (na, na)), self._arr(Qf, (n, n)), self._arr(goal, (P, n) if per else (n,)))
            qc = DojoQuadraticCost(*map(addr, keep), int(per))
        ls = DojoLineSearch(*map(addr, (X, U, status, alpha, dV, ok, Xcur, Ucur, J0, J_trial, J_cur, J_acc, choice, a_acc, Xn, Un)), float(c1), int(act_off), na)
        _chk(lib().dojo_linesearch_select(self.h, H, T, None if qc is None else C.byref(qc), C.byref(ls)))
        out = {"choice": choice, "alpha": a_acc, "J_trial": J_trial, "J_cur": J_cur, "J_acc": J_acc}
        if gather:
            out.update(X=Xn, U=Un)
        return out

    def rollout_policy(self, z0, W, steps, bias=None, mean=None, scale=None, U_ff=None, act_off=0, contact_forces=False, contact_init=0):
        """Closed-loop rollout (dojo_rollout_policy): simulate! with the affine feedback policy u_k = U_ff[k] + E (bias + W ((o_k - mean) .* scale))
        evaluated on the device between the steps, o_k = the observation (`observe`) of the state step k starts from.  W [na, nobs] (one policy
        for all environments) or [B, na, nobs] (one per environment), bias [na] / [B, na], mean, scale [nobs], U_ff [steps, B, nu]; the policy
        drives the inputs act_off .. act_off + na - 1.  Returns (Z [H,B,13Nb], OBS [H+1,B,nobs], U [H,B,nu], status [H,B]): OBS[k] is what the
        policy saw at step k (OBS[H]: the final state's), U[k] what step k was given."""
        B, s = self.batch, self.spec
        H = int(steps)
        z0 = self._arr(z0, (B, s.nz))
        nobs = 2 * s.nu + (len(s.contacts) if contact_forces else 0)
        pol, keep = self._affine_policy(W, bias, mean, scale, U_ff, H, nobs, act_off, contact_forces, contact_init)
        Z, OBS, U, st = self._closed_loop_outputs(H, nobs)
        _chk(lib().dojo_rollout_policy(self.h, addr(z0), C.byref(pol), H, addr(Z), addr(OBS), addr(U), addr(st)))
        return Z, OBS, U, st

    def observation_jacobian(self, z):
        """maximal_to_minimal_jacobian (dojo_observation_jacobian) at z [B,13Nb] -> the COMPACT [B, 2nu, 24] fp64: row i is minimal coordinate i, columns
        0..11 the derivative w.r.t. the tangent coordinates [x; v; phi; omega] of the parent body of the joint that owns the row (0 for a joint on the
        origin), 12..23 w.r.t. those of its child body.  coords.dense_observation_jacobian scatters it to [B, 2nu, 12Nb]."""
        B, s = self.batch, self.spec
        z = self._arr(z, (B, s.nz))
        M = np.empty((B, 2 * s.nu, 24), np.float64)
        _chk(lib().dojo_observation_jacobian(self.h, addr(z), addr(M)))
        return M

    def rollout_policy_gradients(self, z0, W, G, steps=None, bias=None, mean=None, scale=None, U_ff=None, act_off=0, G_u=None, G_obs=None, cot_space="tangent"):
        """Reverse mode through a closed-loop rollout (dojo_rollout_policy_gradients): the rollout of `rollout_policy` (without contact observations) and
        the gradient of a trajectory loss w.r.t. the policy, the feed-forward term and the initial state; the recorded Jacobians stay on the device.
        G [H,B,nx] ("tangent") or [H,B,13Nb] ("state"): cotangent w.r.t. the state after every step; G_u [H,B,nu], G_obs [H+1,B,nobs] (optional):
        w.r.t. the applied controls and the observations.  Returns (Z, OBS, U, status, gW, gbias, gU [H,B,nu], gz0 [B,nx] tangent); gW, gbias have
        the shapes of W, bias ([B,na,nobs] / [B,na] for one policy per environment; [na,nobs] / [na], summed over the batch, for a shared one)."""
        B, s = self.batch, self.spec
        z0 = self._arr(z0, (B, s.nz))
        G, H, cs = self._cotangents("rollout_policy_gradients", G, steps, cot_space)
        nobs = 2 * s.nu
        pol, keep = self._affine_policy(W, bias, mean, scale, U_ff, H, nobs, act_off)
        G_u = None if G_u is None else self._arr(G_u, (H, B, s.nu))
        G_obs = None if G_obs is None else self._arr(G_obs, (H + 1, B, nobs))
        Z, OBS, U, st = self._closed_loop_outputs(H, nobs)
        gW = np.empty_like(keep[0]); gb = np.empty((B, pol.na) if pol.per_env else (pol.na,), self.np_dtype)
        gU = np.empty((H, B, s.nu), self.np_dtype); gz = np.empty((B, s.nx), self.np_dtype)
        _chk(lib().dojo_rollout_policy_gradients(self.h, addr(z0), C.byref(pol), H, addr(G), cs, addr(G_u), addr(G_obs), addr(Z), addr(OBS), addr(U), addr(st),
                                                 addr(gW), addr(gb), addr(gU), addr(gz)))
        return Z, OBS, U, st, gW, gb, gU, gz

    def _mlp_args(self, theta, widths):
        """theta [P] or [B, P] in the handle dtype, the widths as ints, whether there is one policy per environment"""
        w = [int(n) for n in widths]
        P, _ = mlp_sizes(w)
        theta = np.ascontiguousarray(theta, dtype=self.np_dtype)
        if theta.ndim not in (1, 2):
            raise ValueError("theta must be [P] or [B, P]")
        per_env = theta.ndim == 2
        theta = self._arr(theta, (self.batch, P) if per_env else (P,))
        return theta, w, per_env

    def rollout_mlp(self, z0, theta, widths, steps, mean=None, scale=None, U_ff=None, act_off=0, contact_forces=False, contact_init=0):
        """Closed-loop rollout with a tanh network policy (dojo_rollout_mlp): `rollout_policy` with h_l = tanh(b_l + W_l h_{l-1}), h_0 = (o_k - mean) .* scale,
        u_k = U_ff[k] + E (b_L + W_L h_{L-1}) evaluated on the device between the steps.  theta [P] (shared) or [B, P] (one policy per environment) and
        widths [n_0 = nobs, .., n_L = na] as `pack_mlp` returns them.  Returns (Z [H,B,13Nb], OBS [H+1,B,nobs], U [H,B,nu], status [H,B])."""
        B, s = self.batch, self.spec
        H = int(steps)
        z0 = self._arr(z0, (B, s.nz))
        nobs = 2 * s.nu + (len(s.contacts) if contact_forces else 0)
        pol, keep = self._mlp_policy(theta, widths, mean, scale, U_ff, H, nobs, act_off, contact_forces, contact_init)
        Z, OBS, U, st = self._closed_loop_outputs(H, nobs)
        _chk(lib().dojo_rollout_mlp(self.h, addr(z0), C.byref(pol), H, addr(Z), addr(OBS), addr(U), addr(st)))
        return Z, OBS, U, st

    def rollout_mlp_gradients(self, z0, theta, widths, G, steps=None, mean=None, scale=None, U_ff=None, act_off=0, G_u=None, G_obs=None, cot_space="tangent"):
        """Reverse mode through `rollout_mlp` (dojo_rollout_mlp_gradients; without contact observations): the rollout and the gradient of a trajectory
        loss w.r.t. the network's parameters, the feed-forward term and the initial state; the record, the observation Jacobians and the activations
        stay on the device.  Cotangents as in `rollout_policy_gradients`.  Returns (Z, OBS, U, status, gtheta, gU [H,B,nu], gz0 [B,nx] tangent); gtheta
        has the shape of theta ([B, P]; or [P], summed over the batch, for a shared policy)."""
        B, s = self.batch, self.spec
        z0 = self._arr(z0, (B, s.nz))
        G, H, cs = self._cotangents("rollout_mlp_gradients", G, steps, cot_space)
        nobs = 2 * s.nu
        pol, keep = self._mlp_policy(theta, widths, mean, scale, U_ff, H, nobs, act_off)
        G_u = None if G_u is None else self._arr(G_u, (H, B, s.nu))
        G_obs = None if G_obs is None else self._arr(G_obs, (H + 1, B, nobs))
        Z, OBS, U, st = self._closed_loop_outputs(H, nobs)
        gth = np.empty_like(keep[0]); gU = np.empty((H, B, s.nu), self.np_dtype); gz = np.empty((B, s.nx), self.np_dtype)
        _chk(lib().dojo_rollout_mlp_gradients(self.h, addr(z0), C.byref(pol), H, addr(G), cs, addr(G_u), addr(G_obs), addr(Z), addr(OBS), addr(U), addr(st),
                                              addr(gth), addr(gU), addr(gz)))
        return Z, OBS, U, st, gth, gU, gz

    def set_external_force(self, fext):
        """set_external_force!(body; force, torque) for all bodies: fext [B, Nb, 6] = [Fext (world); τext (body frame)],
        None removes them.  In effect for every following step (bodies/set.jl:110-115, constraint.jl:15-18)."""
        if fext is None:
            _chk(lib().dojo_set_external_force(self.h, None)); return
        f = self._arr(np.asarray(fext).reshape(self.batch, 6 * self.spec.Nb), (self.batch, 6 * self.spec.Nb))
        _chk(lib().dojo_set_external_force(self.h, addr(f)))

    def simulate(self, z0, U=None, steps=None):
        """simulate!(mechanism, 1:H, storage, control!; record=true) with pre-sampled controls (simulate.jl:16-37).
        Returns (Z [H,B,13Nb], storage [H,B,Nb,25], status [H,B]); a Storage row is
        x2(3) q2(4) v15(3) w15(3) px(3) pq(3) vl(3) wl(3) of the solved step (storage.jl:50-67), see STORAGE_FIELDS."""
        B, s = self.batch, self.spec
        z0 = self._arr(z0, (B, s.nz))
        U, H = self._controls(U, steps)
        Z = np.empty((H, B, s.nz), self.np_dtype)
        S = np.empty((H, B, s.Nb, 25), self.np_dtype)
        st = np.empty((H, B), np.int32)
        _chk(lib().dojo_simulate(self.h, addr(z0), addr(U), H, addr(Z), addr(S), addr(st)))
        return Z, S, st

    def observe(self, contact_forces=False):
        """get_state(environment): minimal state of the handle's current state [B, 2nu], followed (contact_forces=True,
        get_state(::AntARS), ant_ars.jl:72-80) by the clamped normal impulses of the last step [B, 2nu + Nc]."""
        B, s = self.batch, self.spec
        obs = np.empty((B, 2 * s.nu + (len(s.contacts) if contact_forces else 0)), self.np_dtype)
        _chk(lib().dojo_observe(self.h, addr(obs), int(bool(contact_forces))))
        return obs

    def contact_gradients(self):
        """get_contact_gradients (src/gradients/contact.jl) at the solution of the last step(..., with_gradient=True):
        [B, 12Nb, 5Nc], contact data = [friction_coefficient, contact_radius, contact_origin(3)] per contact."""
        B, s = self.batch, self.spec
        dc = np.zeros((B, s.nx, 5 * len(s.contacts)), self.np_dtype)
        _chk(lib().dojo_contact_gradients(self.h, addr(dc)))
        return dc

    # ---- minimal <-> maximal coordinates (src/mechanism/state.jl:9-66, src/simulation/step.jl:42-60) ----
    def minimal_to_maximal(self, x):
        B, s = self.batch, self.spec
        x = self._arr(x, (B, 2 * s.nu))
        z = np.empty((B, s.nz), self.np_dtype)
        _chk(lib().dojo_minimal_to_maximal(self.h, addr(x), addr(z)))
        return z

    def maximal_to_minimal(self, z):
        B, s = self.batch, self.spec
        z = self._arr(z, (B, s.nz))
        x = np.empty((B, 2 * s.nu), self.np_dtype)
        _chk(lib().dojo_maximal_to_minimal(self.h, addr(z), addr(x)))
        return x

    def step_minimal(self, x, u=None):
        """step_minimal_coordinates!: x [B, 2 nu] -> x_next, status, iters"""
        B, s = self.batch, self.spec
        x = self._arr(x, (B, 2 * s.nu))
        u = self._arr(u, (B, s.nu)) if (u is not None and s.nu) else None
        xn = np.empty((B, 2 * s.nu), self.np_dtype)
        st = np.empty(B, np.int32); it = np.empty(B, np.int32)
        _chk(lib().dojo_step_minimal(self.h, addr(x), addr(u), addr(xn), addr(st), addr(it)))
        return xn, st, it

    def minimal_gradients(self, x, u=None):
        """get_minimal_gradients!: one step in minimal coordinates -> (x_next, status, iters, jx [B,2nu,2nu], ju [B,2nu,nu])"""
        B, s = self.batch, self.spec
        nm = 2 * s.nu
        x = self._arr(x, (B, nm))
        u = self._arr(u, (B, s.nu)) if (u is not None and s.nu) else None
        xn = np.empty((B, nm), self.np_dtype); st = np.empty(B, np.int32); it = np.empty(B, np.int32)
        jx = np.empty((B, nm, nm), self.np_dtype); ju = np.empty((B, nm, max(s.nu, 1)), self.np_dtype)
        _chk(lib().dojo_minimal_gradients(self.h, addr(x), addr(u), addr(xn), addr(st), addr(it), addr(jx), addr(ju)))
        return xn, st, it, jx, ju.reshape(-1)[:B * nm * s.nu].reshape(B, nm, s.nu)

    def last_kernel_ms(self):
        ms = C.c_double(0)
        _chk(lib().dojo_last_kernel_ms(self.h, C.byref(ms)))
        return ms.value

    def kernel_time_totals(self, reset=False):
        """(sum of step-kernel ms, sum of IFT-kernel ms, launches) over the timed launches since the last reset."""
        a = C.c_double(0); b = C.c_double(0); n = C.c_int64(0)
        _chk(lib().dojo_kernel_time_totals(self.h, C.byref(a), C.byref(b), C.byref(n), 1 if reset else 0))
        return a.value, b.value, n.value

    def last_kernel_times(self):
        """(step kernel ms, IFT kernel ms) of the last launch, from hipEvents on the launch stream."""
        a = C.c_double(0); b = C.c_double(0)
        _chk(lib().dojo_last_kernel_times(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value


# ---------------------------------------------------------------------------------------
# Dojo-style free functions
# ---------------------------------------------------------------------------------------
def step(mechanism, z, u=None, opts=None):
    """step!(mechanism, z, u; opts): returns the mechanism's state after the step
    ((x3, v25, q3, ω25) per body -- SURVEY.md §8a Q1), plus per-environment status."""
    if opts is not None:
        mechanism.set_options(opts)
    zn, status, iters = mechanism.step(z, u, with_gradient=False)
    return zn, status


def get_maximal_gradients(mechanism, z, u=None, opts=None):
    """get_maximal_gradients!(mechanism, z, u; opts) -> (jacobian_state [B,12Nb,12Nb], jacobian_control [B,12Nb,nu])"""
    if opts is not None:
        mechanism.set_options(opts)
    mechanism.step(z, u, with_gradient=True)
    return mechanism.gradients()


def simulate(mechanism, z0, U=None, steps=None, opts=None, abort_upon_failure=False):
    """simulate!(mechanism, steps, storage, control!) with pre-sampled controls U[k]."""
    if opts is not None:
        mechanism.set_options(opts)
    return mechanism.rollout(z0, U, steps=steps, record=True)
