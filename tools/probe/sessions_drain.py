"""Timing probe for finishing open calls.

The countdown network at n instances (default 1,048,576), budget 1000.  One
call leaves calls open; that state is snapshotted and restored before every
sample (mk_session_restore_device), so every sample finishes the same calls.
Two open states:

  dense    inputs up to 1023: about two thirds of the calls stay open
  sparse   every sixteenth instance an input up to 1023, the rest up to 63
           (these close within the slice): about 4% stay open

Arms, each finishing every open call of the state:

  host_resume_all     resume() on all n until call_open() is clear
  host_resume_listed  call_open(), then resume(index=open) per slice, the list
                      cut down on the host from the statuses
  drain_host          mk_session_drain
  drain_device        mk_session_drain_device, max_slices = the slices the state needs
  resume_device_all   mk_session_resume_device over all n, once per slice: the
                      kernel work of host_resume_all without its copies

Host arms are wall clock around the (synchronous) calls, device arms HIP
events on a stream around the queued launches.  Every arm is warmed up once,
then `repeats` samples are taken with the arms alternating inside each repeat.

Prints one JSON line per state and arm; --out appends them to a file as well."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import misaka_net_amd as mk  # noqa: E402
from misaka_net_amd import _native as N  # noqa: E402

ARMS = ["host_resume_all", "host_resume_listed", "drain_host", "drain_device", "resume_device_all"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this probe needs a GPU"
    torch.cuda.init()
    n = a.n
    net = mk.Network(mk.networks.countdown_network())
    sess = net.sessions(n, budget=1000)
    plan = sess.plan()
    assert plan.startswith("tier=native"), plan
    lay = sess.layout()
    stream = torch.cuda.Stream()
    sh = stream.cuda_stream

    def inputs(mask, seed):
        x32 = torch.empty(n, dtype=torch.int32, device="cuda")
        mk.generate_inputs_device(n, x32.data_ptr(), seed=seed, gen_kind=1, gen_mask=mask, stream=sh)
        torch.cuda.synchronize()
        return x32.to(torch.int64)

    big, small = inputs(1023, 0x4D49534B41), inputs(63, 0x4D49534B42)
    sparse = small.clone()
    sparse[::16] = big[::16]
    out = torch.empty(n, dtype=torch.int32, device="cuda")
    st = torch.empty(n, dtype=torch.uint8, device="cuda")
    sp = torch.empty(n, dtype=torch.int32, device="cuda")
    left = torch.zeros(1, dtype=torch.int32, device="cuda")

    lines = []
    for state, x in (("dense", big), ("sparse", sparse)):
        sess.reset()
        sess.compute_device(x.data_ptr(), out.data_ptr(), st.data_ptr(), None, stream=sh)
        rec = torch.zeros(lay.rows * n, dtype=torch.int32, device="cuda")
        sess.snapshot_device(rec.data_ptr(), stream=sh)
        torch.cuda.synchronize()
        opened = int(sess.call_open().sum())

        def restore():
            sess.restore_device(lay, rec.data_ptr(), n, stream=sh)
            torch.cuda.synchronize()

        # the slices the state needs, and the answer every arm must leave behind
        ref = sess.drain(max_slices=64)
        assert ref.still_open == 0
        slices = 0
        restore()
        while sess.call_open().any():
            sess.resume()
            slices += 1
        assert slices >= 1

        def run(arm):
            """One sample: microseconds to finish every open call of the restored state."""
            if arm in ("drain_device", "resume_device_all"):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                if arm == "drain_device":
                    sess.drain_device(slices, out.data_ptr(), st.data_ptr(), sp.data_ptr(), left.data_ptr(), stream=sh)
                else:
                    for _ in range(slices):
                        sess.resume_device(out.data_ptr(), st.data_ptr(), sp.data_ptr(), stream=sh)
                e1.record(stream)
                torch.cuda.synchronize()
                return e0.elapsed_time(e1) * 1e3
            t0 = time.perf_counter()
            if arm == "host_resume_all":
                while sess.call_open().any():
                    sess.resume()
            elif arm == "host_resume_listed":
                todo = np.flatnonzero(sess.call_open())
                while todo.size:
                    r = sess.resume(index=todo)
                    todo = todo[r.status == N.MK_ST_BUDGET]
            else:
                r = sess.drain(max_slices=64)
                assert r.still_open == 0
            return (time.perf_counter() - t0) * 1e6

        samples = {arm: [] for arm in ARMS}
        for rep in range(a.repeats + 1):  # the first round warms every arm up
            for arm in ARMS:
                restore()
                t = run(arm)
                assert not sess.call_open().any(), arm
                if arm == "drain_device":
                    assert int(left.item()) == 0
                    assert np.array_equal(out.cpu().numpy(), ref.out) and np.array_equal(st.cpu().numpy(), ref.status)
                    assert np.array_equal(sp.cpu().numpy().astype(np.uint32), ref.steps)
                if rep:
                    samples[arm].append(t)
        for arm in ARMS:
            v = samples[arm]
            med = statistics.median(v)
            lines.append({"probe": "sessions_drain", "state": state, "arm": arm, "n": n, "open": opened,
                          "slices": slices, "us_median": round(med, 1), "us_min": round(min(v), 1),
                          "us_max": round(max(v), 1), "us_per_slice_median": round(med / slices, 1),
                          "repeats": a.repeats, "samples_us": [round(t, 1) for t in v], "plan": plan})
    sess.close()
    for ln in lines:
        print(json.dumps(ln))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
