"""Session snapshots on the host model (sched_check.cpp mkc_sess_export_idle,
mkc_sess_copy): schedcheck.HostSessions with the record conversion of a live
session between calls and the native raw copy, so both are checked on the CPU."""
import ctypes as C

import numpy as np

import schedcheck as sc


class SnapSessions(sc.HostSessions):
    def __init__(self, nodes, n, *, stack_cap=None):
        super().__init__(nodes, n, stack_cap=stack_cap)
        h = sc.lib()
        h.mkc_sess_export_idle.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(sc.OrcFlat), C.c_void_p]
        h.mkc_sess_copy.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t]

    def export_idle(self, i, nstack):
        """Session i (live, no hand-off) through its canonical record, in the
        oracle's terms: (OrcFlat, its entries buffer)."""
        f = sc.OrcFlat()
        ent = np.zeros(max(1, nstack) * self.cap, np.int32)
        rc = sc.lib().mkc_sess_export_idle(self._h, i, C.byref(f), ent.ctypes.data)
        assert rc == 0, f"idle export error {rc} (session {i})"
        f.entries = ent.ctypes.data
        return f, ent

    def copy(self, dst, src):
        assert sc.lib().mkc_sess_copy(self._h, dst, src) == 0
