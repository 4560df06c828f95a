"""ctypes wrapper of tests/emu/libcoords_emu.so: the per-joint coordinate templates of dojo.jl_amd/csrc/dojo_coords.hpp (double and Dual<24>)
compiled with g++, for one environment.  Test infrastructure only."""
import ctypes as C
import os
import numpy as np
from emu_wrap import _build, _p

_HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None


def lib():
    global _lib
    if _lib is None:
        so = os.path.join(_HERE, "emu", "libcoords_emu.so")
        src = [os.path.join(_HERE, "emu", "coords_emu.cpp")] + [os.path.join(_HERE, "..", "dojo.jl_amd", "csrc", f)
                                                                for f in ("dojo_coords.hpp", "dojo_host.hpp", "dojo_entries.hpp", "dojo_device.hpp", "dojo_math.hpp")]
        _build(so, src)
        _lib = C.CDLL(so)
        for f in ("coords_min2max", "coords_max2min", "coords_min2max_jacobian", "coords_max2min_jacobian"):
            getattr(_lib, f).restype = C.c_int
    return _lib


class CoordsEmu:
    """the host instantiation of the device's coordinate templates for one MechanismSpec"""

    def __init__(self, spec):
        self.spec = spec
        self._topo, self._keep = spec.to_ctypes()

    def _call(self, name, *arrays):
        rc = getattr(lib(), name)(C.byref(self._topo), *[_p(a) for a in arrays])
        if rc != 0:
            raise RuntimeError("%s: %d" % (name, rc))

    def minimal_to_maximal(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64); z = np.zeros(13 * self.spec.Nb)
        self._call("coords_min2max", x, z)
        return z

    def maximal_to_minimal(self, z):
        z = np.ascontiguousarray(z, dtype=np.float64); x = np.zeros(2 * self.spec.nu)
        self._call("coords_max2min", z, x)
        return x

    def minimal_to_maximal_jacobian(self, x, z=None):
        """[12Nb, 2nu] at x; the parents' states are read from z (min2max_jac_kernel's second buffer), minimal_to_maximal(x) unless given"""
        x = np.ascontiguousarray(x, dtype=np.float64)
        z = self.minimal_to_maximal(x) if z is None else np.ascontiguousarray(z, dtype=np.float64)
        J = np.zeros((12 * self.spec.Nb, 2 * self.spec.nu))
        self._call("coords_min2max_jacobian", x, z, J)
        return J

    def maximal_to_minimal_jacobian(self, z):
        """[2nu, 12Nb] at z"""
        z = np.ascontiguousarray(z, dtype=np.float64)
        J = np.zeros((2 * self.spec.nu, 12 * self.spec.Nb))
        self._call("coords_max2min_jacobian", z, J)
        return J
