"""Host-side mirror of the reference's node network for the batched /compute path.

``Network`` replaces the set of ``ProgramNode``/``StackNode`` processes of a
deployment (internal/nodes/program.go, internal/nodes/stack.go; topology from
NODE_INFO, cmd/app.go:31, and each node's PROGRAM, cmd/app.go:21) by one
loaded ``mk_net`` handle.  ``compute_batch`` evaluates many independent
``/compute`` inputs (master.go:197-224) at once on the GPU.
"""
from __future__ import annotations

import atexit
import ctypes as C
import weakref
from dataclasses import dataclass
from typing import Iterable, Mapping, Optional, Sequence

import numpy as np

from . import _native as N

STATUS_NAMES = {
    N.MK_ST_QUIESCENT: "quiescent",
    N.MK_ST_BUDGET: "budget",
    N.MK_ST_STACK_OVERFLOW: "stack_overflow",
    N.MK_ST_OUTPUT_STOP: "output_stop",
}


# Native handles still open at interpreter exit are freed by an atexit hook
# (sessions before the networks they run on), while the HIP runtime and the
# caller's GPU state are intact, instead of by garbage collection during
# teardown or never.
_LIVE: "weakref.WeakSet" = weakref.WeakSet()


@atexit.register
def _close_live():
    live = list(_LIVE)
    for o in [o for o in live if isinstance(o, SessionSet)] + [o for o in live if isinstance(o, Network)]:
        try:
            o.close()
        except Exception:  # pragma: no cover - best effort at exit
            pass


def _ptr(a):
    """A host array as the C ABI takes it; None is the null pointer."""
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class TisParseError(ValueError):
    """A program was rejected; ``str(e)`` is the reference's Go error text."""


def tokenize(program: str) -> list[list[str]]:
    """tis.Tokenize (internal/tis/tokenizer.go:29-106) on one program: the
    ``[][]string`` the reference builds, or TisParseError with its message."""
    buf = C.create_string_buffer(max(4096, 64 * len(program) + 1024))
    rc = N.lib().mk_tokenize(program.encode(), buf, len(buf))
    text = buf.value.decode(errors="surrogateescape")
    if rc == N.MK_EPARSE:
        raise TisParseError(text)
    N.check(rc, "mk_tokenize")
    return [line.split("\x1f") for line in text.split("\n")]


@dataclass
class NodeSpec:
    name: str
    kind: str = "program"  # "program" | "stack" | "master" | "remote_program" | "remote_stack"
    program: str = ""


_KINDS = {"program": N.MK_NODE_PROGRAM, "stack": N.MK_NODE_STACK, "master": N.MK_NODE_MASTER,
          "remote_program": N.MK_NODE_REMOTE_PROGRAM, "remote_stack": N.MK_NODE_REMOTE_STACK}


@dataclass
class BatchResult:
    out: np.ndarray  # int32: first OUT value (the /compute result), 0 if none
    status: np.ndarray  # uint8: MK_ST_* reason | MK_ST_HAS_OUTPUT
    steps: Optional[np.ndarray]  # uint32 retired node-instructions, if requested
    still_open: Optional[int] = None  # SessionSet.drain and serve: calls left open at the slice limit
    rounds: Optional[int] = None  # SessionSet.serve: ragged launches made
    ids: Optional[np.ndarray] = None  # SessionDirectory: uint32, the instance of each request (0xffffffff: none)
    counts: Optional[tuple] = None  # SessionDirectory: keys admitted, keys rejected, requests of rejected keys
    evicted_keys: Optional[np.ndarray] = None  # SessionDirectory with evict: the victims' keys (then counts[3]: their number)
    evicted_ids: Optional[np.ndarray] = None  # and their instances, increasing

    @property
    def has_output(self) -> np.ndarray:
        return (self.status & N.MK_ST_HAS_OUTPUT) != 0

    @property
    def reason(self) -> np.ndarray:
        return self.status & N.MK_ST_REASON_MASK


_MODES = {None: 0, "interp": N.MK_FLAG_FORCE_INTERP, "tile": N.MK_FLAG_TILE, "refill": N.MK_FLAG_REFILL,
          "jit": N.MK_FLAG_JIT}


def make_opts(budget=None, stack_cap=None, stop_on_output=False, devices: Optional[Iterable[int]] = None,
              interp=False, mode=None):
    """mk_opts.  ``mode``: None (automatic), "jit" (demand the native
    per-network kernel, tier 3), "tile" or "refill" (the tier-2 superblock
    interpreter with that lane scheduling, see mk.h MK_FLAG_TILE), "interp"
    (the direct bytecode interpreter, tier 1; same as ``interp=True``)."""
    if mode not in _MODES:
        raise ValueError(f"unknown executor mode {mode!r}")
    o = N.mk_opts()
    o.budget = int(budget or 0)
    o.stack_cap = int(stack_cap or 0)
    o.flags = ((N.MK_FLAG_STOP_ON_OUTPUT if stop_on_output else 0) | (N.MK_FLAG_FORCE_INTERP if interp else 0)
               | _MODES[mode])
    mask = 0
    for d in devices or ():
        mask |= 1 << int(d)
    o.device_mask = mask
    return o


class Network:
    """A loaded network.

    ``nodes`` is a sequence of NodeSpec (or ``(name, kind, program)`` tuples).
    Program nodes are executed in sorted-name order (the canonical schedule).
    """

    def __init__(self, nodes: Sequence):
        specs = [n if isinstance(n, NodeSpec) else NodeSpec(*n) for n in nodes]
        arr = (N.mk_node_desc * len(specs))()
        self._keep = []
        for i, s in enumerate(specs):
            if s.kind not in _KINDS:
                raise ValueError(f"invalid node type {s.kind!r}")
            nm, pg = s.name.encode(), (s.program or "").encode()
            self._keep += [nm, pg]
            arr[i].name, arr[i].kind, arr[i].program = nm, _KINDS[s.kind], pg
        h = C.c_void_p()
        err = C.create_string_buffer(8192)
        rc = N.lib().mk_net_load(arr, len(specs), C.byref(h), err, len(err))
        if rc == N.MK_EPARSE:
            raise TisParseError(err.value.decode(errors="surrogateescape"))
        N.check(rc, err.value.decode(errors="surrogateescape"))
        self._h = h
        self.specs = specs
        _LIVE.add(self)

    @classmethod
    def from_node_info(cls, node_info: Mapping[str, Mapping], programs: Mapping[str, str], master: Optional[str] = None):
        """Build from the master's NODE_INFO JSON (docker-compose.yml:16-21) and
        each program node's PROGRAM env var (cmd/app.go:21)."""
        nodes = [NodeSpec(name, info["type"], programs.get(name, "")) for name, info in node_info.items()]
        if master:
            nodes.append(NodeSpec(master, "master"))
        return cls(nodes)

    def close(self):
        if getattr(self, "_h", None):
            N.lib().mk_net_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self) -> C.c_void_p:
        return self._h

    def info(self):
        c = (C.c_int * 3)()
        N.check(N.lib().mk_net_info(self._h, c))
        return {"program_nodes": c[0], "stack_nodes": c[1], "instructions": c[2]}

    def disasm(self) -> str:
        buf = C.create_string_buffer(1 << 20)
        N.check(N.lib().mk_net_disasm(self._h, buf, len(buf)))
        return buf.value.decode()

    def plan(self, *, stack_cap=None, stop_on_output=False, interp=False, mode=None) -> str:
        """Which executor tier runs this network (compiles the schedule, and
        the native kernel, once)."""
        buf = C.create_string_buffer(4096)
        o = make_opts(None, stack_cap, stop_on_output, None, interp, mode)
        rc = N.lib().mk_net_plan(self._h, C.byref(o), buf, len(buf))
        if rc == N.MK_ELIMIT:
            return buf.value.decode()
        N.check(rc)
        return buf.value.decode()

    def prepare(self, *, stack_cap=None, stop_on_output=False, mode=None, device=0):
        """Compile everything a launch with these options uses on ``device``."""
        o = make_opts(None, stack_cap, stop_on_output, None, False, mode)
        N.check(N.lib().mk_net_prepare(self._h, C.byref(o), device), self.plan(stack_cap=stack_cap,
                                                                             stop_on_output=stop_on_output, mode=mode))

    def jit_source(self, *, stack_cap=None, stop_on_output=False) -> str:
        """hiprtc source of the native (tier-3) kernel."""
        buf = C.create_string_buffer(1 << 24)
        o = make_opts(None, stack_cap, stop_on_output)
        rc = N.lib().mk_net_jit_source(self._h, C.byref(o), buf, len(buf))
        N.check(rc, buf.value.decode())
        return buf.value.decode()

    def sched_disasm(self, *, stack_cap=None, stop_on_output=False) -> str:
        buf = C.create_string_buffer(1 << 24)
        o = make_opts(None, stack_cap, stop_on_output)
        N.check(N.lib().mk_net_sched_disasm(self._h, C.byref(o), buf, len(buf)))
        return buf.value.decode()

    def compute_batch(self, values, *, budget=None, stack_cap=None, stop_on_output=False, devices=None, steps=True,
                      interp=False, mode=None):
        """Evaluate independent /compute inputs (strconv.Atoi int64 values,
        truncated to int32 at GetInput like master.go:237) on the GPU(s)."""
        v = np.ascontiguousarray(np.asarray(values, dtype=np.int64))
        n = v.size
        out = np.zeros(n, np.int32)
        st = np.zeros(n, np.uint8)
        sp = np.zeros(n, np.uint32) if steps else None
        o = make_opts(budget, stack_cap, stop_on_output, devices, interp, mode)
        rc = N.lib().mk_compute_batch(
            self._h,
            _ptr(v),
            n,
            _ptr(out),
            _ptr(st),
            _ptr(sp),
            C.byref(o),
        )
        N.check(rc, "mk_compute_batch")
        return BatchResult(out, st, sp)

    def compute_device(self, n, *, out_ptr, status_ptr, steps_ptr=None, stats_ptr=None, device=0, stream=None,
                       in_ptr=None, in_kind=N.MK_IN_I32, seed=0, gen_kind=N.MK_GEN_FULL, gen_mask=0, offset=0,
                       budget=None, stack_cap=None, stop_on_output=False, interp=False, mode=None,
                       defer_stats=False):
        """Launch on device memory (raw pointers, e.g. torch ``data_ptr()``);
        asynchronous on ``stream`` (a HIP stream handle, e.g.
        ``torch.cuda.current_stream().cuda_stream``).  ``defer_stats``: keep
        this launch's counters on the device until :meth:`stats_fold`."""
        mi = N.mk_input()
        mi.kind = N.MK_IN_GEN if in_ptr is None else in_kind
        mi.data = in_ptr
        mi.seed = seed
        mi.gen_kind = gen_kind
        mi.gen_mask = gen_mask
        mi.offset = offset
        o = make_opts(budget, stack_cap, stop_on_output, None, interp, mode)
        if defer_stats:
            o.flags |= N.MK_FLAG_DEFER_STATS
        rc = N.lib().mk_compute_device(
            self._h, device, C.byref(mi), n, out_ptr, status_ptr, steps_ptr, stats_ptr, C.byref(o), stream
        )
        N.check(rc, "mk_compute_device")

    def device_launcher(self, n, *, out_ptr, status_ptr, steps_ptr=None, device=0, in_ptr=None,
                        in_kind=N.MK_IN_I32, seed=0, gen_kind=N.MK_GEN_FULL, gen_mask=0, offset=0, budget=None,
                        stack_cap=None, stop_on_output=False, mode=None, defer_stats=False):
        """``compute_device`` with every argument fixed: returns ``launch(stream)``
        whose host cost is one foreign call (the ctypes structs are built once)."""
        mi = N.mk_input()
        mi.kind = N.MK_IN_GEN if in_ptr is None else in_kind
        mi.data = in_ptr
        mi.seed = seed
        mi.gen_kind = gen_kind
        mi.gen_mask = gen_mask
        mi.offset = offset
        o = make_opts(budget, stack_cap, stop_on_output, None, False, mode)
        if defer_stats:
            o.flags |= N.MK_FLAG_DEFER_STATS
        fn, h, pmi, po = N.lib().mk_compute_device, self._h, C.byref(mi), C.byref(o)

        def launch(stream=None):
            rc = fn(h, device, pmi, n, out_ptr, status_ptr, steps_ptr, None, po, stream)
            if rc:
                N.check(rc, "mk_compute_device")

        launch.keep = (mi, o, self)
        return launch

    TRACE_DTYPE = np.dtype([("round", "<u4"), ("node", "<u2"), ("ip", "<u2"), ("acc", "<i8"), ("bak", "<i8")])

    def trace(self, value, *, max_entries=4096, budget=None, stack_cap=None, stop_on_output=False, device=0):
        """Lane trace of one /compute input (mk_trace_lane): the first
        ``max_entries`` retired instructions as a structured array
        (round, node, ip, acc, bak) and the lane's status byte."""
        out = np.zeros(max_entries, self.TRACE_DTYPE)
        cnt = C.c_uint32()
        st = C.c_uint8()
        o = make_opts(budget, stack_cap, stop_on_output)
        N.check(N.lib().mk_trace_lane(self._h, device, int(value), C.byref(o), _ptr(out),
                                      max_entries, C.byref(cnt), C.byref(st)), "mk_trace_lane")
        return out[: cnt.value], st.value

    def sessions(self, n, *, device=0, budget=None, stack_cap=None) -> "SessionSet":
        """``n`` stateful instances of this network (row f2, :class:`SessionSet`)."""
        return SessionSet(self, n, device=device, budget=budget, stack_cap=stack_cap)

    def stats_fold(self, stats_ptr, *, device=0, stream=None):
        """Add the counters of deferred launches on ``device`` into the
        device uint64[MK_STATS_LEN] at ``stats_ptr`` (asynchronous)."""
        N.check(N.lib().mk_stats_fold(self._h, device, stats_ptr, stream), "mk_stats_fold")


class SessionSet:
    """``n`` stateful instances of a network on one GPU (SURVEY.md section 8
    row f2).  The reference's nodes keep running between /compute calls
    (program.go:80-92); here each instance's ACC/BAK/ptr, ports, stacks and the
    master's inChan/outChan persist in HBM between calls, and :meth:`compute`
    performs one /compute (master.go:216-219) on every instance at once."""

    def __init__(self, net: "Network", n: int, *, device: int = 0, budget=None, stack_cap=None):
        o = make_opts(budget, stack_cap)
        h = C.c_void_p()
        N.check(N.lib().mk_session_create(net.handle, device, n, C.byref(o), C.byref(h)), "mk_session_create")
        self._h, self._net, self.n, self.device = h, net, n, device
        _LIVE.add(self)

    def _index(self, index) -> np.ndarray:
        """An index list as the C ABI takes it (uint32, strictly increasing,
        every entry < n); ValueError names the first offending position."""
        a = np.asarray(index)
        if a.size and a.dtype.kind not in "iu":
            raise ValueError(f"index must hold integers, got dtype {a.dtype}")
        a = a.reshape(-1).astype(np.int64) if a.size else np.zeros(0, np.int64)
        if a.size > self.n:
            raise ValueError(f"index position {self.n}: more than the set's {self.n} instances listed")
        bad = (a < 0) | (a >= self.n)
        bad[1:] |= a[1:] <= a[:-1]
        if bad.any():
            t = int(np.argmax(bad))
            why = "is not an instance" if not 0 <= a[t] < self.n else f"does not exceed position {t - 1}'s {a[t - 1]}"
            raise ValueError(f"index position {t}: {a[t]} {why} (n = {self.n}; strictly increasing)")
        return np.ascontiguousarray(a.astype(np.uint32))

    def compute(self, values, *, steps=True, busy_ok=False, index=None) -> BatchResult:
        """One /compute call per instance: ``values[i]`` goes to instance i.

        A call whose budget slice runs out stays open (status MK_ST_BUDGET):
        :meth:`resume` continues it, :meth:`cancel` abandons it.  While one is
        open a new call on that instance does nothing (MK_ST_CALL_OPEN) and
        this raises MkError(MK_EBUSY) unless ``busy_ok``.

        With ``index`` (strictly increasing instance numbers) only the listed
        instances take a call: ``values[t]`` goes to instance ``index[t]``,
        results have ``len(index)`` columns, and every other instance stays
        exactly as it was."""
        v = np.ascontiguousarray(np.asarray(values, dtype=np.int64))
        if index is not None:
            sel = self._index(index)
            if v.size != sel.size:
                raise ValueError(f"expected {sel.size} values, got {v.size}")
            return self._call("mk_session_step_indexed", sel.size, steps, busy_ok, _ptr(sel), sel.size, _ptr(v))
        if v.size != self.n:
            raise ValueError(f"expected {self.n} values, got {v.size}")
        return self._call("mk_session_compute", self.n, steps, busy_ok, _ptr(v))

    def resume(self, *, steps=True, index=None) -> BatchResult:
        """One more budget slice of every instance's open call (instances
        without one report status 0) -- mk_session_step(in = NULL); with
        ``index``, of the listed instances' open calls only."""
        if index is not None:
            sel = self._index(index)
            return self._call("mk_session_step_indexed", sel.size, steps, False, _ptr(sel), sel.size, None)
        return self._call("mk_session_step", self.n, steps, False, None)

    def _call(self, name, shape, steps, busy_ok, *args, tail=()) -> BatchResult:
        """One host form of the C ABI, ``N.lib().<name>(set, *args, out, status,
        steps, *tail)``, into fresh result arrays of ``shape``.  MkError names
        ``name``; MK_EBUSY passes with ``busy_ok``."""
        out = np.zeros(shape, np.int32)
        st = np.zeros(shape, np.uint8)
        sp = np.zeros(shape, np.uint32) if steps else None
        rc = getattr(N.lib(), name)(self._h, *args, _ptr(out), _ptr(st), _ptr(sp), *tail)
        if not (busy_ok and rc == N.MK_EBUSY):
            N.check(rc, name)
        return BatchResult(out, st, sp)

    def plan(self) -> str:
        """Which tier runs the sessions (mk_session_plan)."""
        buf = C.create_string_buffer(1024)
        N.check(N.lib().mk_session_plan(self._h, buf, len(buf)), "mk_session_plan")
        return buf.value.decode()

    def cancel(self, *, index=None):
        """Abandon every instance's open call (mk_session_cancel); with
        ``index``, the listed instances' only."""
        if index is not None:
            sel = self._index(index)
            N.check(N.lib().mk_session_cancel_indexed(self._h, _ptr(sel), sel.size),
                    "mk_session_cancel_indexed")
            return
        N.check(N.lib().mk_session_cancel(self._h), "mk_session_cancel")

    def call_open(self, index=None) -> np.ndarray:
        """Which instances have a call open (uint8, 1 = open): all ``n``, or
        the listed ones in the order of ``index`` (mk_session_call_open)."""
        sel = self._index(index) if index is not None else None
        m = self.n if sel is None else sel.size
        op = np.zeros(m, np.uint8)
        N.check(N.lib().mk_session_call_open(self._h, _ptr(sel), m, _ptr(op)), "mk_session_call_open")
        return op

    # ---- open calls (include/mk.h: the list, the device resume and the drain) ----
    def _listed(self, index_ptr, m) -> int:
        if (index_ptr is None) != (m is None):
            raise ValueError("index_ptr and m go together")
        if m is None:
            return self.n
        if not 0 <= m <= self.n:
            raise ValueError(f"m = {m} outside [0, {self.n}]")
        return m

    def open_list(self, index=None):
        """The instances with a call open, found and packed on the GPU
        (mk_session_open_list): ``(list, pos)``, uint32 arrays of as many
        entries as there are open calls among all ``n`` instances or the
        listed ones.  ``list`` is increasing -- itself a valid ``index`` --
        and ``index[pos[k]] == list[k]`` (without ``index``, ``pos`` is
        ``list``)."""
        sel = self._index(index) if index is not None else None
        m = self.n if sel is None else sel.size
        lst, pos = np.zeros(m, np.uint32), np.zeros(m, np.uint32)
        cnt = C.c_size_t()
        N.check(N.lib().mk_session_open_list(self._h, _ptr(sel), m, _ptr(lst), _ptr(pos), C.byref(cnt)),
                "mk_session_open_list")
        return lst[:cnt.value], pos[:cnt.value]

    def open_list_device(self, list_ptr, pos_ptr, count_ptr, *, stream=None, index_ptr=None, m=None):
        """:meth:`open_list` into device uint32 arrays of ``m`` entries
        (``pos_ptr`` may be None) and one count word, asynchronous on
        ``stream``.  Past the count the list is padded with 0xffffffff and
        ``pos`` with 0, so the list serves as the ``index_ptr`` of a launch
        over ``m`` entries without reading the count back.  ``index_ptr`` and
        ``m`` as in :meth:`compute_device`."""
        m = self._listed(index_ptr, m)
        N.check(N.lib().mk_session_open_list_device(self._h, index_ptr, m, list_ptr, pos_ptr, count_ptr, stream),
                "mk_session_open_list_device")

    def resume_device(self, out_ptr, status_ptr, steps_ptr=None, *, stream=None, index_ptr=None, m=None):
        """:meth:`resume` on device arrays of ``m`` columns, asynchronous on
        ``stream`` (mk_session_resume_device); ``index_ptr`` and ``m`` as in
        :meth:`compute_device`."""
        m = self._listed(index_ptr, m)
        N.check(N.lib().mk_session_resume_device(self._h, index_ptr, m, out_ptr, status_ptr, steps_ptr, stream),
                "mk_session_resume_device")

    def drain(self, *, index=None, max_slices=16, steps=True, promote=False) -> BatchResult:
        """Finish the open calls of every instance, or of the listed ones:
        what :meth:`resume` on them, then again on those still at MK_ST_BUDGET,
        up to ``max_slices`` times in all would report -- each instance the
        result of its last slice, one without an open call what a resume
        reports for it (mk_session_drain).  On the GPU every slice runs over a
        packed list of the calls still open, not over the whole set.
        ``still_open`` of the result counts the calls left open at the limit.
        With ``promote`` the instances go back to the native tier afterwards
        (:meth:`promote` on the same ``index``)."""
        if int(max_slices) < 1:
            raise ValueError(f"max_slices = {max_slices}: at least one slice")
        if int(max_slices) >= 1 << 32:
            raise ValueError(f"max_slices = {max_slices}: 2^32 or more")
        sel = self._index(index) if index is not None else None
        m = self.n if sel is None else sel.size
        left = C.c_size_t()
        r = self._call("mk_session_drain", m, steps, False, _ptr(sel), m, int(max_slices), tail=(C.byref(left),))
        r.still_open = left.value
        if promote:
            self.promote(index)
        return r

    def drain_device(self, max_slices, out_ptr, status_ptr, steps_ptr=None, still_open_ptr=None, *, stream=None,
                     index_ptr=None, m=None):
        """:meth:`drain` on device arrays of ``m`` columns, asynchronous on
        ``stream`` and without any read-back: all ``max_slices`` slices are
        queued (mk_session_drain_device).  ``still_open_ptr`` (one device
        uint32, or None) takes the number of calls left open."""
        if not 1 <= int(max_slices) < 1 << 32:
            raise ValueError(f"max_slices = {max_slices} outside [1, 2^32)")
        m = self._listed(index_ptr, m)
        N.check(N.lib().mk_session_drain_device(self._h, index_ptr, m, int(max_slices), out_ptr, status_ptr,
                                                steps_ptr, still_open_ptr, stream), "mk_session_drain_device")

    def compute_seq(self, values, *, steps=True, busy_ok=False, index=None) -> BatchResult:
        """Sequential /compute calls in one launch: ``values`` has shape
        (ncalls, n) -- row c is call c on every instance -- or, for n == 1,
        a flat list of the calls.  Results have the shape of ``values``.  A
        call that stays open (MK_ST_BUDGET) makes the instance's later calls
        of the burst report MK_ST_CALL_OPEN without running."""
        v = np.ascontiguousarray(np.asarray(values, dtype=np.int64))
        shape = v.shape
        if index is not None:
            # values and results (ncalls, len(index)): column t is instance index[t]
            sel = self._index(index)
            if v.ndim != 2 or v.shape[1] != sel.size:
                raise ValueError(f"expected (ncalls, {sel.size}) values, got {shape}")
            return self._call("mk_session_compute_indexed", shape, steps, busy_ok, _ptr(sel), sel.size, _ptr(v),
                              shape[0])
        if v.ndim == 1 and self.n == 1:
            v = v.reshape(-1, 1)
        if v.ndim != 2 or v.shape[1] != self.n:
            raise ValueError(f"expected (ncalls, {self.n}) values, got {shape}")
        return self._call("mk_session_compute_seq", shape, steps, busy_ok, _ptr(v), v.shape[0])

    def compute_device(self, in_ptr, out_ptr, status_ptr, steps_ptr=None, *, stream=None, index_ptr=None, m=None):
        """One call on device arrays, asynchronous on ``stream``.  With
        ``index_ptr`` (a device uint32 array of ``m`` strictly increasing
        instance numbers, taken on trust and to be kept unchanged until the
        launch completes) the arrays have ``m`` columns and only the listed
        instances take the call (mk_session_compute_indexed_device)."""
        if index_ptr is not None:
            return self.compute_seq_device(in_ptr, 1, out_ptr, status_ptr, steps_ptr, stream=stream,
                                           index_ptr=index_ptr, m=m)
        if m is not None:
            raise ValueError("m goes with index_ptr")
        N.check(N.lib().mk_session_compute_device(self._h, in_ptr, out_ptr, status_ptr, steps_ptr, stream),
                "mk_session_compute_device")

    def compute_seq_device(self, in_ptr, ncalls, out_ptr, status_ptr, steps_ptr=None, *, stream=None, index_ptr=None,
                           m=None):
        """A burst of `ncalls` sequential calls per instance in one launch on
        device arrays laid out [call][instance] (mk_session_compute_seq_device);
        with ``index_ptr`` and ``m`` as in :meth:`compute_device`, laid out
        [call][m]."""
        if (index_ptr is None) != (m is None):
            raise ValueError("index_ptr and m go together")
        if index_ptr is not None:
            if not 0 <= m <= self.n:
                raise ValueError(f"m = {m} outside [0, {self.n}]")
            N.check(N.lib().mk_session_compute_indexed_device(self._h, index_ptr, m, in_ptr, ncalls, out_ptr,
                                                              status_ptr, steps_ptr, stream),
                    "mk_session_compute_indexed_device")
            return
        N.check(N.lib().mk_session_compute_seq_device(self._h, in_ptr, ncalls, out_ptr, status_ptr, steps_ptr, stream),
                "mk_session_compute_seq_device")

    @staticmethod
    def _ragged(values, counts):
        """A ragged burst's flat inputs and offsets (uint32, ``m + 1`` of
        them) from ``values`` and ``counts``; ValueError names the first
        offending position."""
        if counts is None:
            rows = [np.asarray(r, dtype=np.int64).reshape(-1) for r in values]
            cnt = np.array([r.size for r in rows], np.int64)
            v = np.concatenate(rows) if rows else np.zeros(0, np.int64)
        else:
            c = np.asarray(counts).reshape(-1)
            if c.size and c.dtype.kind not in "iu":
                each = list(counts) if not isinstance(counts, np.ndarray) else list(c)
                t = next((i for i, x in enumerate(each) if not isinstance(x, (int, np.integer)) or
                          isinstance(x, (bool, np.bool_))), 0)
                raise ValueError(f"counts position {t}: {each[t]!r} is not an integer")
            cnt = c.astype(np.int64) if c.size else np.zeros(0, np.int64)
            if (cnt < 0).any():
                t = int(np.argmax(cnt < 0))
                raise ValueError(f"counts position {t}: {cnt[t]} is negative")
            v = np.asarray(values, dtype=np.int64).reshape(-1)
        off = np.zeros(cnt.size + 1, np.int64)
        np.cumsum(cnt, out=off[1:])
        if off[-1] >= 1 << 32:
            t = int(np.argmax(off[1:] >= 1 << 32))
            raise ValueError(f"counts position {t}: the calls up to here number {off[t + 1]}, 2^32 or more")
        if v.size != off[-1]:
            # the entry whose calls the values end in, or past the last entry
            t = int(np.searchsorted(off[1:], v.size, side="right")) if v.size < off[-1] else cnt.size
            raise ValueError(f"counts position {t}: {v.size} values for {int(off[-1])} calls "
                             f"(len(values) != sum(counts))")
        return np.ascontiguousarray(v), np.ascontiguousarray(off.astype(np.uint32))

    def compute_ragged(self, values, counts=None, *, index=None, steps=True, busy_ok=False) -> BatchResult:
        """A ragged burst in one launch: entry t makes ``counts[t]`` sequential
        /compute calls on instance ``index[t]`` (t itself without ``index``),
        exactly as that many :meth:`compute` calls on it alone would
        (mk_session_compute_ragged).  With ``counts``, ``values`` is flat and
        entry-major -- entry t's inputs at ``sum(counts[:t])`` onwards --
        and without, a sequence of per-entry sequences.  The result holds flat
        arrays in the same order.  An entry with count 0 is not touched.
        MkError(MK_EBUSY) unless ``busy_ok`` when a listed instance with a
        call to make had one open."""
        v, off = self._ragged(values, counts)
        sel = self._index(index) if index is not None else None
        m = self.n if sel is None else sel.size
        if off.size - 1 != m:
            raise ValueError(f"expected {m} entries, got {off.size - 1}")
        return self._call("mk_session_compute_ragged", int(off[-1]), steps, busy_ok, _ptr(sel), m, _ptr(off), _ptr(v))

    def compute_ragged_device(self, in_ptr, off_ptr, total, out_ptr, status_ptr, steps_ptr=None, *, stream=None,
                              index_ptr=None, m=None):
        """A ragged burst on device arrays, asynchronous on ``stream``
        (mk_session_compute_ragged_device): ``off_ptr`` is a device uint32
        array of ``m + 1`` offsets (0 first, non-decreasing, ``total`` last),
        the I/O arrays hold ``total`` words, entry-major.  ``index_ptr`` and
        ``m`` as in :meth:`compute_device`; without them every instance is
        listed.  Offsets and list are taken on trust and kept unchanged until
        the launch completes."""
        if (index_ptr is None) != (m is None):
            raise ValueError("index_ptr and m go together")
        if m is None:
            m = self.n
        if not 0 <= m <= self.n:
            raise ValueError(f"m = {m} outside [0, {self.n}]")
        if not 0 <= total < 1 << 32:
            raise ValueError(f"total = {total} outside [0, 2^32)")
        N.check(N.lib().mk_session_compute_ragged_device(self._h, index_ptr, m, off_ptr, total, in_ptr, out_ptr,
                                                         status_ptr, steps_ptr, stream),
                "mk_session_compute_ragged_device")

    def _queue(self, ids, values):
        """A request queue as the C ABI takes it (uint32 ids, every one < n,
        int64 values of the same length); ValueError names the first offending
        position."""
        raw = ids if isinstance(ids, np.ndarray) else list(ids)
        a = np.asarray(raw).reshape(-1)
        if a.size and a.dtype.kind not in "iu":
            each = list(a) if isinstance(raw, np.ndarray) else raw
            t = next((i for i, x in enumerate(each) if not isinstance(x, (int, np.integer)) or
                      isinstance(x, (bool, np.bool_))), 0)
            raise ValueError(f"ids position {t}: {each[t]!r} is not an integer")
        a = a.astype(np.int64) if a.size and a.dtype != np.uint64 else a
        if a.size == 0:
            a = np.zeros(0, np.int64)
        bad = (a < 0) | (a >= self.n)
        if bad.any():
            t = int(np.argmax(bad))
            raise ValueError(f"ids position {t}: {a[t]} is not an instance (n = {self.n})")
        v = np.asarray(values, dtype=np.int64).reshape(-1)
        if v.size != a.size:
            t = min(v.size, a.size)
            raise ValueError(f"ids position {t}: {a.size} ids for {v.size} values (len(ids) != len(values))")
        if a.size >= 1 << 32:
            raise ValueError(f"ids position {(1 << 32) - 1}: 2^32 requests or more")
        return np.ascontiguousarray(a.astype(np.uint32)), np.ascontiguousarray(v)

    def compute_queue(self, ids, values, *, steps=True, busy_ok=False) -> BatchResult:
        """A request queue in arrival order in one launch: request j is one
        /compute call with ``values[j]`` on instance ``ids[j]`` -- any order,
        repeats allowed -- and the results come back in that same order,
        exactly as if the requests had been served one at a time
        (mk_session_compute_queue).  The grouping by instance runs on the GPU.
        The requests of one instance follow the rules of a burst
        (:meth:`compute_ragged`); an instance with no request is not touched.
        MkError(MK_EBUSY) unless ``busy_ok`` when the first request of an
        instance found a call open."""
        q, v = self._queue(ids, values)
        return self._call("mk_session_compute_queue", q.size, steps, busy_ok, _ptr(q), _ptr(v), q.size)

    def compute_queue_device(self, ids_ptr, in_ptr, total, out_ptr, status_ptr, steps_ptr=None, *, stream=None):
        """A request queue on device arrays of ``total`` words each,
        asynchronous on ``stream`` (mk_session_compute_queue_device).  The
        ids (uint32) are taken on trust; a request whose id is ``>= n``
        touches no instance and reports 0 / 0 / 0."""
        if not 0 <= total < 1 << 32:
            raise ValueError(f"total = {total} outside [0, 2^32)")
        N.check(N.lib().mk_session_compute_queue_device(self._h, ids_ptr, in_ptr, total, out_ptr, status_ptr,
                                                        steps_ptr, stream),
                "mk_session_compute_queue_device")

    # ---- served queues (include/mk.h: a request queue answered to completion) ----
    @staticmethod
    def _slices(name, value):
        if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)):
            raise ValueError(f"{name} = {value!r} is not an integer")
        if not 1 <= int(value) < 1 << 32:
            raise ValueError(f"{name} = {value} outside [1, 2^32)")
        return int(value)

    def serve(self, ids, values, *, max_slices=16, steps=True, busy_ok=False, promote=False) -> BatchResult:
        """A request queue served to completion on the GPU: what
        :meth:`compute_queue` answers when every call that outlives its budget
        slice is resumed, up to ``max_slices`` more slices as :meth:`drain`
        gives it, before the next request of its instance runs -- the requests
        of one instance one at a time, each waiting for its answer
        (mk_session_serve).  A call still open after its slices stays open
        (MK_ST_BUDGET) and the later requests of its instance report
        MK_ST_CALL_OPEN; an instance whose call was open beforehand is not
        resumed, all its requests report MK_ST_CALL_OPEN, and this raises
        MkError(MK_EBUSY) unless ``busy_ok``.  ``still_open`` of the result
        counts the requests left at MK_ST_BUDGET, ``rounds`` the ragged
        launches made.  With ``promote`` the instances go back to the native
        tier afterwards (:meth:`promote` on the whole set)."""
        k = SessionSet._slices("max_slices", max_slices)
        q, v = SessionSet._queue(self, ids, values)
        left, rounds = C.c_size_t(), C.c_size_t()
        r = self._call("mk_session_serve", q.size, steps, busy_ok, _ptr(q), _ptr(v), q.size, k,
                       tail=(C.byref(left), C.byref(rounds)))
        r.still_open, r.rounds = left.value, rounds.value
        if promote:
            self.promote()
        return r

    def serve_device(self, ids_ptr, in_ptr, total, max_slices, max_rounds, out_ptr, status_ptr, steps_ptr=None,
                     left_ptr=None, *, stream=None):
        """:meth:`serve` on device arrays of ``total`` words each, asynchronous
        on ``stream`` and without any read-back: exactly ``max_rounds`` rounds
        are queued (mk_session_serve_device).  A request no round reached is
        unserved and reports 0 / 0 / 0; the unserved requests of an instance
        are the last of its requests, so serving them again in order continues
        the queue.  ``left_ptr`` (two device uint32, or None) takes the numbers
        of requests left open and unserved.  The ids (uint32) are taken on
        trust; one that is ``>= n`` touches no instance, reports 0 / 0 / 0 and
        is not counted."""
        k = SessionSet._slices("max_slices", max_slices)
        nr = SessionSet._slices("max_rounds", max_rounds)
        if not 0 <= total < 1 << 32:
            raise ValueError(f"total = {total} outside [0, 2^32)")
        N.check(N.lib().mk_session_serve_device(self._h, ids_ptr, in_ptr, total, k, nr, out_ptr, status_ptr, steps_ptr,
                                                left_ptr, stream), "mk_session_serve_device")

    def reset(self, *, index=None):
        """/reset (master.go:126-143): every instance back to its initial
        state; with ``index``, the listed instances only."""
        if index is not None:
            sel = self._index(index)
            N.check(N.lib().mk_session_reset_indexed(self._h, _ptr(sel), sel.size),
                    "mk_session_reset_indexed")
            return
        N.check(N.lib().mk_session_reset(self._h), "mk_session_reset")

    def reset_device(self, index_ptr, m, stream=None):
        """:meth:`reset` of the ``m`` instances listed in the device uint32
        array ``index_ptr`` (strictly increasing, taken on trust; an entry
        ``>= n`` touches nothing), asynchronous on ``stream``
        (mk_session_reset_indexed_device)."""
        if not 0 <= m <= self.n:
            raise ValueError(f"m = {m} outside [0, {self.n}]")
        N.check(N.lib().mk_session_reset_indexed_device(self._h, index_ptr, m, stream),
                "mk_session_reset_indexed_device")

    # ---- client keys (include/mk.h: a directory from 64-bit keys to instances) ----
    def directory(self) -> "SessionDirectory":
        """The set's directory from client keys to instances, opened on first
        use (mk_session_dir_open: that resets the set and frees every
        instance)."""
        d = getattr(self, "_dir", None)
        if d is None:
            N.check(N.lib().mk_session_dir_open(self._h), "mk_session_dir_open")
            d = self._dir = SessionDirectory(self)
        return d

    # ---- snapshots (include/mk.h: a session's state out of the set and back) ----
    def layout(self) -> "N.mk_session_layout":
        """What a block of this set's session records looks like (mk_session_layout_get)."""
        lay = N.mk_session_layout()
        N.check(N.lib().mk_session_layout_get(self._h, C.byref(lay)), "mk_session_layout_get")
        return lay

    def snapshot(self, index=None) -> "SessionSnapshot":
        """The whole state of every instance, or of the listed ones (column t
        is instance ``index[t]``): registers, ports, stacks, inChan / outChan,
        the open call and the tier that holds it.  Reads the set, changes nothing."""
        sel = self._index(index) if index is not None else None
        m = self.n if sel is None else sel.size
        lay = self.layout()
        rec = np.zeros((lay.rows, m), np.uint32)
        N.check(N.lib().mk_session_snapshot(self._h, _ptr(sel), m, _ptr(rec)), "mk_session_snapshot")
        return SessionSnapshot(lay, rec)

    def _layout_fits(self, lay):
        own = self.layout()
        for f in ("magic", "version", "net_hash", "nprog", "nstack", "stack_cap"):
            if getattr(lay, f) != getattr(own, f):
                raise ValueError(f"snapshot layout mismatch in {f}: the snapshot's {getattr(lay, f)}, "
                                 f"this set's {getattr(own, f)}")
        if lay.rows != own.rows - own.native_rows + lay.native_rows:
            raise ValueError(f"snapshot layout mismatch in rows: {lay.rows} is not what its sections add up to")

    def restore(self, snap: "SessionSnapshot", index=None, take=None):
        """Overwrite every instance, or the listed ones, with records of
        ``snap``: instance ``index[t]`` takes column ``take[t]`` (column t
        without ``take``).  The snapshot may come from another set, GPU or
        tier of the same network and stack_cap; a record goes back to the
        native tier only in a set running the same native module, otherwise
        the interpreter holds that instance until promoted.  ValueError, with
        nothing changed, for a layout of another network or a record out of
        range."""
        sel = self._index(index) if index is not None else None
        m = self.n if sel is None else sel.size
        self._layout_fits(snap.layout)
        rec = np.ascontiguousarray(snap.rec, dtype=np.uint32)
        if rec.ndim != 2 or rec.shape[0] != snap.layout.rows:
            raise ValueError(f"snapshot block has shape {rec.shape}, its layout {snap.layout.rows} rows")
        mcols = rec.shape[1]
        col = None
        if take is not None:
            a = np.asarray(take)
            if a.size and a.dtype.kind not in "iu":
                raise ValueError(f"take must hold integers, got dtype {a.dtype}")
            a = a.reshape(-1).astype(np.int64) if a.size else np.zeros(0, np.int64)
            if a.size != m:
                raise ValueError(f"take names {a.size} columns for {m} instances")
            bad = (a < 0) | (a >= mcols)
            if bad.any():
                t = int(np.argmax(bad))
                raise ValueError(f"take position {t}: {a[t]} is not a column of the snapshot's {mcols}")
            col = np.ascontiguousarray(a.astype(np.uint32))
        elif m > mcols:
            raise ValueError(f"take position {mcols}: the snapshot has {mcols} columns for {m} instances")
        rc = N.lib().mk_session_restore(self._h, _ptr(sel), m, C.byref(snap.layout), _ptr(rec), mcols, _ptr(col))
        if rc == N.MK_EINVAL:
            raise ValueError("snapshot record out of range (held, an ip, a stack depth or the native superblock): "
                             "nothing restored")
        N.check(rc, "mk_session_restore")

    def fork(self, src: int, index):
        """Copy instance ``src`` into the listed instances: they continue
        from its state, each on its own."""
        if not 0 <= int(src) < self.n:
            raise ValueError(f"fork source {src} is not an instance (n = {self.n})")
        sel = self._index(index)
        self.restore(self.snapshot(index=[int(src)]), index=sel, take=np.zeros(sel.size, np.int64))

    def snapshot_device(self, rec_ptr, *, stream=None, index_ptr=None, m=None):
        """:meth:`snapshot` into a device uint32 block [rows][m] (``rows``
        from :meth:`layout`), asynchronous on ``stream``; ``index_ptr`` and
        ``m`` as in :meth:`compute_device`."""
        if (index_ptr is None) != (m is None):
            raise ValueError("index_ptr and m go together")
        N.check(N.lib().mk_session_snapshot_device(self._h, index_ptr, self.n if m is None else m, rec_ptr, stream),
                "mk_session_snapshot_device")

    def restore_device(self, layout, rec_ptr, mcols, *, stream=None, index_ptr=None, m=None, take_ptr=None):
        """:meth:`restore` from a device block of ``mcols`` columns described
        by ``layout``, asynchronous on ``stream``.  The block, ``index_ptr``
        and ``take_ptr`` (device uint32 arrays of ``m`` entries) are taken on
        trust; an entry out of range restores nothing."""
        if (index_ptr is None) != (m is None):
            raise ValueError("index_ptr and m go together")
        self._layout_fits(layout)
        N.check(N.lib().mk_session_restore_device(self._h, index_ptr, self.n if m is None else m, C.byref(layout),
                                                  rec_ptr, mcols, take_ptr, stream), "mk_session_restore_device")

    # ---- promotion (include/mk.h: interpreter-held instances back to the native tier) ----
    def promote(self, index=None) -> np.ndarray:
        """Hand every instance the interpreter holds between calls back to the
        native tier, or the listed ones only; bool flags in list order, True
        where the instance was promoted (mk_session_promote).  An instance
        with a call open, one the native tier already holds, and one whose
        state a cancel left outside every call-start state report False and
        stay as they are.  Later calls return what they would have anyway."""
        sel = self._index(index) if index is not None else None
        m = self.n if sel is None else sel.size
        flags = np.zeros(m, np.uint8)
        N.check(N.lib().mk_session_promote(self._h, _ptr(sel), m, _ptr(flags), None), "mk_session_promote")
        return flags.astype(bool)

    def promote_device(self, flags_ptr, *, stream=None, index_ptr=None, m=None):
        """:meth:`promote` on device arrays, asynchronous on ``stream``:
        ``flags_ptr`` (a device uint8 array of ``m`` entries, or None) takes
        the flags; ``index_ptr`` and ``m`` as in :meth:`compute_device`."""
        if (index_ptr is None) != (m is None):
            raise ValueError("index_ptr and m go together")
        N.check(N.lib().mk_session_promote_device(self._h, index_ptr, self.n if m is None else m, flags_ptr, stream),
                "mk_session_promote_device")

    def close(self):
        if getattr(self, "_h", None):
            N.lib().mk_session_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


KEY_NONE = (1 << 64) - 1  # MK_KEY_NONE: the key that is never bound
NO_INSTANCE = 0xFFFFFFFF  # the id of a request that touches no instance


class SessionDirectory:
    """The directory of a :class:`SessionSet` from 64-bit client keys to its
    instances, kept on the GPU with a FIFO of the free instances (include/mk.h,
    client keys).  A new key takes the instance at the front of the FIFO, which
    is in the post-/reset state; :meth:`release` resets a departed client's
    instance and puts it at the back.  Every integer in ``[0, 2^64)`` is a
    key; :data:`KEY_NONE` marks a request of no client, which is never bound
    and never served.  From :meth:`SessionSet.directory`."""

    def __init__(self, sset: "SessionSet"):
        self._set = sset

    @property
    def _h(self):
        if getattr(self._set, "_dir", None) is not self:
            raise ValueError("this directory has been closed")
        return self._set._h

    @staticmethod
    def _keys(keys, values=None):
        """Keys as the C ABI takes them (uint64; with ``values``, int64 of the
        same length beside them); ValueError names the first offending
        position."""
        if isinstance(keys, np.ndarray) and keys.dtype.kind != "O":
            a = keys.reshape(-1)
            if a.size and a.dtype.kind not in "iu":
                raise ValueError(f"keys position 0: {a[0]!r} is not an integer (dtype {a.dtype})")
            if a.size and a.dtype.kind == "i" and (a < 0).any():
                t = int(np.argmax(a < 0))
                raise ValueError(f"keys position {t}: {a[t]} is negative")
            k = a.astype(np.uint64) if a.size else np.zeros(0, np.uint64)
        else:
            each = list(keys.reshape(-1)) if isinstance(keys, np.ndarray) else list(keys)
            for t, x in enumerate(each):
                if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, np.integer)):
                    raise ValueError(f"keys position {t}: {x!r} is not an integer")
                if x < 0:
                    raise ValueError(f"keys position {t}: {x} is negative")
                if x >= 1 << 64:
                    raise ValueError(f"keys position {t}: {x} is 2^64 or more")
            k = np.array([int(x) for x in each], dtype=np.uint64)
        if k.size >= 1 << 32:
            raise ValueError(f"keys position {(1 << 32) - 1}: 2^32 keys or more")
        k = np.ascontiguousarray(k)
        if values is None:
            return k
        v = np.asarray(values, dtype=np.int64).reshape(-1)
        if v.size != k.size:
            t = min(v.size, k.size)
            raise ValueError(f"keys position {t}: {k.size} keys for {v.size} values (len(keys) != len(values))")
        return k, np.ascontiguousarray(v)

    def bind(self, keys, evict=None, min_idle=1):
        """The instance of every key, in arrival order, new keys admitted
        (mk_session_bind): ``(ids, counts)`` -- uint32 ids, 0xffffffff for
        :data:`KEY_NONE` and for a key rejected because no instance was free,
        and ``counts = (keys admitted, keys rejected, requests of rejected
        keys)``.  New keys take the free instances in the order of their first
        occurrence.

        With ``evict`` (a tracked directory, :meth:`track`) the bind makes
        room: when the new keys outnumber the free instances, up to ``evict``
        of the clients silent longest -- at least ``min_idle`` binds, no call
        open -- are evicted first (mk_session_bind_evict).  The result is then
        ``(ids, counts, evicted_keys, evicted_ids)`` with the number evicted as
        ``counts[3]`` and the victims in increasing instance order."""
        k = self._keys(keys)
        ids = np.zeros(k.size, np.uint32)
        if evict is None:
            c = (C.c_size_t * 3)()
            N.check(N.lib().mk_session_bind(self._h, _ptr(k), k.size, _ptr(ids), c), "mk_session_bind")
            return ids, tuple(int(x) for x in c)
        want, idle = self._want("evict", evict), self._want("min_idle", min_idle)
        cap = min(want, self._set.n)
        ek, ei = np.full(cap, KEY_NONE, np.uint64), np.full(cap, NO_INSTANCE, np.uint32)
        c = (C.c_size_t * 4)()
        N.check(N.lib().mk_session_bind_evict(self._h, _ptr(k), k.size, _ptr(ids), want, idle, _ptr(ek), _ptr(ei), c),
                "mk_session_bind_evict")
        return ids, tuple(int(x) for x in c), ek[:c[3]], ei[:c[3]]

    @staticmethod
    def _want(name, value):
        if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)):
            raise ValueError(f"{name} = {value!r} is not an integer")
        if not 0 <= int(value) < 1 << 32:
            raise ValueError(f"{name} = {value} outside [0, 2^32)")
        return int(value)

    def track(self):
        """Turn use tracking on (mk_session_dir_track): from now on every bind
        stamps the instances it resolves to with the directory's clock, the
        number of binds so far.  ValueError on a second call."""
        rc = N.lib().mk_session_dir_track(self._h)
        if rc == N.MK_EINVAL:
            raise ValueError("this directory is tracked already")
        N.check(rc, "mk_session_dir_track")

    def use_info(self) -> "N.mk_session_dir_use_info":
        """``clock`` and ``tracking`` of the directory."""
        i = N.mk_session_dir_use_info()
        N.check(N.lib().mk_session_dir_use_info_get(self._h, C.byref(i)), "mk_session_dir_use_info_get")
        return i

    def _select(self, name, want, min_idle):
        want, idle = self._want("want", want), self._want("min_idle", min_idle)
        cap = min(want, self._set.n)
        keys, ids = np.full(cap, KEY_NONE, np.uint64), np.full(cap, NO_INSTANCE, np.uint32)
        c = C.c_size_t()
        N.check(getattr(N.lib(), name)(self._h, want, idle, _ptr(keys), _ptr(ids), C.byref(c)), name)
        return keys[:c.value], ids[:c.value]

    def idle(self, want, min_idle=1):
        """The ``want`` clients silent longest (mk_session_idle_select):
        ``(keys, ids)`` in increasing instance order, fewer when fewer are
        eligible -- bound, at least ``min_idle`` binds since the last one that
        named them, no call open.  Changes nothing.  To park them:
        ``snapshot(index=ids)``, then ``release(keys)``."""
        return self._select("mk_session_idle_select", want, min_idle)

    def evict(self, want, min_idle=1):
        """:meth:`idle`, and the selected clients are released
        (mk_session_evict): ``(keys, ids)`` of the victims."""
        return self._select("mk_session_evict", want, min_idle)

    def export_use(self):
        """``(last, clock)``: the use stamp of every instance (uint64, 0 for a
        free one) and the directory's clock."""
        last = np.zeros(self._set.n, np.uint64)
        clock = C.c_uint64()
        N.check(N.lib().mk_session_dir_use_export(self._h, _ptr(last), C.byref(clock)), "mk_session_dir_use_export")
        return last, clock.value

    def load_use(self, last, clock):
        """Replace the use stamps and the clock by what :meth:`export_use`
        gave (after :meth:`load`).  ValueError, with nothing changed, when a
        bound instance has a stamp above ``clock``."""
        a = np.ascontiguousarray(np.asarray(last, dtype=np.uint64).reshape(-1))
        if a.size != self._set.n:
            raise ValueError(f"last position {min(a.size, self._set.n)}: {a.size} stamps for {self._set.n} instances")
        if not 0 <= clock < 1 << 64:
            raise ValueError(f"clock = {clock} outside [0, 2^64)")
        rc = N.lib().mk_session_dir_use_import(self._h, _ptr(a), clock)
        if rc == N.MK_EINVAL:
            raise ValueError("untracked, or a stamp above the clock: nothing loaded")
        N.check(rc, "mk_session_dir_use_import")

    def _evicting(self, form, keys, values, evict, min_idle, **kw):
        """bind_evict, then the unkeyed ``form`` on the requests that got an
        instance; the others report 0 / 0 / 0."""
        k, v = self._keys(keys, values)
        ids, counts, ek, ei = self.bind(k, evict=evict, min_idle=min_idle)
        got = ids != NO_INSTANCE
        steps = kw.get("steps", True)
        r = BatchResult(np.zeros(k.size, np.int32), np.zeros(k.size, np.uint8),
                        np.zeros(k.size, np.uint32) if steps else None)
        part = getattr(self._set, form)(ids[got], v[got], **kw)
        r.out[got], r.status[got] = part.out, part.status
        if steps:
            r.steps[got] = part.steps
        r.still_open, r.rounds = part.still_open, part.rounds
        r.ids, r.counts, r.evicted_keys, r.evicted_ids = ids, counts, ek, ei
        return r

    def lookup(self, keys) -> np.ndarray:
        """As :meth:`bind`, but nothing is admitted: an unbound key gives
        0xffffffff (mk_session_lookup)."""
        k = self._keys(keys)
        ids = np.zeros(k.size, np.uint32)
        N.check(N.lib().mk_session_lookup(self._h, _ptr(k), k.size, _ptr(ids)), "mk_session_lookup")
        return ids

    def release(self, keys) -> int:
        """Unbind the listed keys, reset their instances and put them at the
        back of the FIFO in increasing order; the number released
        (mk_session_release).  Unbound keys and repeats are ignored."""
        k = self._keys(keys)
        r = C.c_size_t()
        N.check(N.lib().mk_session_release(self._h, _ptr(k), k.size, C.byref(r)), "mk_session_release")
        return r.value

    def compute_queue(self, keys, values, *, steps=True, busy_ok=False, evict=None, min_idle=1) -> BatchResult:
        """:meth:`bind`, then :meth:`SessionSet.compute_queue` on the ids, in
        one call with the keys staged once (mk_session_compute_queue_keyed).
        The result also carries ``ids`` and ``counts``; the requests of
        rejected keys and of :data:`KEY_NONE` report 0 / 0 / 0.  With
        ``evict`` the bind makes room as :meth:`bind` describes (two calls:
        mk_session_bind_evict, then the unkeyed queue on the ids), and the
        result carries ``evicted_keys`` and ``evicted_ids`` too."""
        if evict is not None:
            return self._evicting("compute_queue", keys, values, evict, min_idle, steps=steps,
                                  busy_ok=busy_ok)
        k, v = self._keys(keys, values)
        ids = np.zeros(k.size, np.uint32)
        c = (C.c_size_t * 3)()
        r = SessionSet._call(self, "mk_session_compute_queue_keyed", k.size, steps, busy_ok, _ptr(k), _ptr(v), k.size,
                             tail=(_ptr(ids), c))
        r.ids, r.counts = ids, tuple(int(x) for x in c)
        return r

    def serve(self, keys, values, *, max_slices=16, steps=True, busy_ok=False, promote=False, evict=None,
              min_idle=1) -> BatchResult:
        """:meth:`bind`, then :meth:`SessionSet.serve` on the ids
        (mk_session_serve_keyed); the result also carries ``ids`` and
        ``counts``.  ``evict`` as in :meth:`compute_queue`."""
        if evict is not None:
            return self._evicting("serve", keys, values, evict, min_idle, max_slices=max_slices, steps=steps,
                                  busy_ok=busy_ok, promote=promote)
        n = SessionSet._slices("max_slices", max_slices)
        k, v = self._keys(keys, values)
        ids = np.zeros(k.size, np.uint32)
        c = (C.c_size_t * 3)()
        left, rounds = C.c_size_t(), C.c_size_t()
        r = SessionSet._call(self, "mk_session_serve_keyed", k.size, steps, busy_ok, _ptr(k), _ptr(v), k.size, n,
                             tail=(_ptr(ids), c, C.byref(left), C.byref(rounds)))
        r.ids, r.counts = ids, tuple(int(x) for x in c)
        r.still_open, r.rounds = left.value, rounds.value
        if promote:
            self._set.promote()
        return r

    def export(self) -> np.ndarray:
        """The key of every instance (uint64, :data:`KEY_NONE` for a free one)."""
        owner = np.zeros(self._set.n, np.uint64)
        N.check(N.lib().mk_session_dir_export(self._h, _ptr(owner)), "mk_session_dir_export")
        return owner

    def load(self, owner):
        """Replace the whole directory by an array as :meth:`export` gives it;
        no instance is reset, and the free instances queue up in increasing
        order.  ValueError, with nothing changed, when a key occurs twice."""
        o = self._keys(owner)
        if o.size != self._set.n:
            raise ValueError(f"owner position {min(o.size, self._set.n)}: {o.size} keys for {self._set.n} instances")
        rc = N.lib().mk_session_dir_import(self._h, _ptr(o))
        if rc == N.MK_EINVAL:
            raise ValueError("a key occurs twice: nothing loaded")
        N.check(rc, "mk_session_dir_import")

    def info(self) -> "N.mk_session_dir_info":
        """``slots``, ``live``, ``free`` and ``tombstones`` of the directory."""
        i = N.mk_session_dir_info()
        N.check(N.lib().mk_session_dir_info_get(self._h, C.byref(i)), "mk_session_dir_info_get")
        return i

    def close(self):
        """Drop the directory; the instances stay as they are."""
        if getattr(self._set, "_dir", None) is self:
            N.check(N.lib().mk_session_dir_close(self._set._h), "mk_session_dir_close")
            self._set._dir = None

    @staticmethod
    def _total(total):
        if not 0 <= total < 1 << 32:
            raise ValueError(f"total = {total} outside [0, 2^32)")
        return total

    def bind_device(self, keys_ptr, total, ids_ptr, counts_ptr=None, *, stream=None):
        """:meth:`bind` on device arrays (uint64 keys, uint32 ids, three uint32
        counts or None), asynchronous on ``stream`` and without any read-back
        (mk_session_bind_device).  The ids feed
        :meth:`SessionSet.compute_queue_device` and ``serve_device`` as they are."""
        N.check(N.lib().mk_session_bind_device(self._h, keys_ptr, self._total(total), ids_ptr, counts_ptr, stream),
                "mk_session_bind_device")

    def bind_evict_device(self, keys_ptr, total, ids_ptr, max_evict, *, min_idle=1, ev_keys_ptr=None, ev_ids_ptr=None,
                          counts_ptr=None, stream=None):
        """:meth:`bind` with ``evict`` on device arrays, asynchronous on
        ``stream`` (mk_session_bind_evict_device): the victims' lists take
        ``min(max_evict, n)`` entries each (or None), ``counts_ptr`` four
        uint32 words (or None)."""
        N.check(N.lib().mk_session_bind_evict_device(self._h, keys_ptr, self._total(total), ids_ptr,
                                                     self._want("max_evict", max_evict),
                                                     self._want("min_idle", min_idle), ev_keys_ptr, ev_ids_ptr,
                                                     counts_ptr, stream), "mk_session_bind_evict_device")

    def idle_device(self, want, keys_ptr, ids_ptr, count_ptr=None, *, min_idle=1, stream=None):
        """:meth:`idle` into device arrays of ``min(want, n)`` entries each,
        padded; ``count_ptr`` (one device uint32, or None) takes the number
        (mk_session_idle_select_device)."""
        N.check(N.lib().mk_session_idle_select_device(self._h, self._want("want", want),
                                                      self._want("min_idle", min_idle), keys_ptr, ids_ptr, count_ptr,
                                                      stream), "mk_session_idle_select_device")

    def evict_device(self, want, keys_ptr=None, ids_ptr=None, count_ptr=None, *, min_idle=1, stream=None):
        """:meth:`evict` on the device, asynchronous on ``stream``; every array
        may be None (mk_session_evict_device)."""
        N.check(N.lib().mk_session_evict_device(self._h, self._want("want", want), self._want("min_idle", min_idle),
                                                keys_ptr, ids_ptr, count_ptr, stream), "mk_session_evict_device")

    def lookup_device(self, keys_ptr, total, ids_ptr, *, stream=None):
        """:meth:`lookup` on device arrays, asynchronous on ``stream``."""
        N.check(N.lib().mk_session_lookup_device(self._h, keys_ptr, self._total(total), ids_ptr, stream),
                "mk_session_lookup_device")

    def release_device(self, keys_ptr, m, released_ptr=None, *, stream=None):
        """:meth:`release` of ``m`` device keys, asynchronous on ``stream``;
        ``released_ptr`` (one device uint32, or None) takes the number released."""
        N.check(N.lib().mk_session_release_device(self._h, keys_ptr, self._total(m), released_ptr, stream),
                "mk_session_release_device")


def directory_slots(n) -> int:
    """The table size of a directory for ``n`` instances (mk_session_dir_slots)."""
    s = C.c_uint32()
    N.check(N.lib().mk_session_dir_slots(n, C.byref(s)), "mk_session_dir_slots")
    return s.value


def directory_home(keys, slots) -> np.ndarray:
    """Where each key's probe starts in a table of ``slots`` slots (mk_session_dir_home)."""
    k = SessionDirectory._keys(keys)
    home = np.zeros(k.size, np.uint32)
    N.check(N.lib().mk_session_dir_home(_ptr(k), k.size, slots, _ptr(home)), "mk_session_dir_home")
    return home


class SessionSnapshot:
    """Session records out of a :class:`SessionSet` (include/mk.h, snapshots):
    ``layout`` describes the block, ``rec`` is uint32[rows, m], column t one
    instance's whole state."""

    _HEAD = np.dtype("<u8")

    def __init__(self, layout, rec):
        self.layout, self.rec = layout, rec

    @property
    def m(self) -> int:
        return self.rec.shape[1]

    @property
    def held(self) -> np.ndarray:
        """Per record: the native tier held the instance (the interpreter: False)."""
        return self.rec[0] == 1

    def canonical(self, t: int) -> dict:
        """Record t's canonical part, in the bytecode interpreter's terms."""
        lay, r = self.layout, self.rec[:, t]

        def i32(a):
            return np.asarray(a, np.uint32).view(np.int32)

        def i64(lo, hi):
            return (np.asarray(lo, np.uint64) | (np.asarray(hi, np.uint64) << np.uint64(32))).view(np.int64)

        node = r[9:9 + 10 * lay.nprog].reshape(lay.nprog, 10)
        stacks = r[9 + 10 * lay.nprog:9 + 10 * lay.nprog + lay.nstack * (1 + lay.stack_cap)]
        stacks = stacks.reshape(lay.nstack, 1 + lay.stack_cap)
        io = int(r[1])
        return dict(
            held=int(r[0]), io=io, in_full=io & 1, out_full=(io >> 1) & 1, undeposited=(io >> 2) & 1,
            call_open=(io >> 3) & 1, dead=(io >> 4) & 15, csteps=int(r[2]), pin=int(i32(r[3:4])[0]),
            in_val=int(i32(r[4:5])[0]), out_val=int(i32(r[5:6])[0]), pend=int(r[6]) & 0xFFFF, hung=int(r[6]) >> 16,
            pfull=int(r[7]) | int(r[8]) << 32, acc=i64(node[:, 0], node[:, 1]), bak=i64(node[:, 2], node[:, 3]),
            ip=i32(node[:, 4]).copy(), pendv=i32(node[:, 5]).copy(), port=i32(node[:, 6:10]).copy(),
            depth=stacks[:, 0].copy(), entries=i32(stacks[:, 1:]).copy())

    def tobytes(self) -> bytes:
        """The snapshot as bytes (layout, column count, block), for :meth:`frombytes`."""
        return bytes(self.layout) + np.array([self.m], self._HEAD).tobytes() + \
            np.ascontiguousarray(self.rec, dtype="<u4").tobytes()

    @classmethod
    def frombytes(cls, b: bytes) -> "SessionSnapshot":
        k = C.sizeof(N.mk_session_layout)
        if len(b) < k + 8:
            raise ValueError("not a session snapshot: too short")
        lay = N.mk_session_layout.from_buffer_copy(b[:k])
        m = int(np.frombuffer(b[k:k + 8], cls._HEAD)[0])
        if lay.magic != 0x52534B4D or len(b) != k + 8 + 4 * lay.rows * m:
            raise ValueError("not a session snapshot: bad magic or size")
        return cls(lay, np.frombuffer(b[k + 8:], "<u4").reshape(lay.rows, m).astype(np.uint32))


def generate_inputs_device(n, out_ptr, *, seed, gen_kind=N.MK_GEN_FULL, gen_mask=0, offset=0, device=0, stream=None):
    N.check(N.lib().mk_generate_inputs_device(device, seed, gen_kind, gen_mask, offset, n, out_ptr, stream))


def valu_probe_device(blocks, iters, *, device=0, stream=None) -> int:
    ops = C.c_uint64()
    N.check(N.lib().mk_valu_probe_device(device, blocks, iters, C.byref(ops), stream))
    return ops.value


def group_requests_tmp_bytes(n, total) -> int:
    """Bytes of device scratch :func:`group_requests_device` needs for
    ``total`` requests on ``n`` sessions (mk_requests_group_tmp_bytes)."""
    b = C.c_size_t()
    if not 0 <= n < 1 << 32 or total < 0:
        raise ValueError(f"n = {n}, total = {total}")
    N.check(N.lib().mk_requests_group_tmp_bytes(n, total, C.byref(b)), "mk_requests_group_tmp_bytes")
    return b.value


def group_requests_device(n, ids_ptr, total, perm_ptr, sel_ptr, off_ptr, m_ptr, tmp_ptr, tmp_bytes, *, device=0,
                          stream=None):
    """Group a request queue on the GPU, asynchronous on ``stream``
    (mk_requests_group_device): from ``total`` uint32 ids in arrival order,
    the stable order ``perm`` of ``min(id, n)``, the distinct ids below ``n``
    (``sel``, ``min(total, n)`` words, padded with 0xffffffff), where each
    one's requests start in that order (``off``, one word more, padded with
    the number of valid requests) and their number (``m``, one word)."""
    if not 0 <= n < 1 << 32 or total < 0:
        raise ValueError(f"n = {n}, total = {total}")
    N.check(N.lib().mk_requests_group_device(device, n, ids_ptr, total, perm_ptr, sel_ptr, off_ptr, m_ptr, tmp_ptr,
                                             tmp_bytes, stream), "mk_requests_group_device")
