"""Timing probe for served request queues.

The countdown network at n instances (default 1,048,576), budget 150, and a
queue of `total` requests (default 4 * n) with uniformly random ids and inputs
up to 1023.  Every sample starts from a reset set and serves the whole queue.
Arms:

  serve_device   mk_session_serve_device, max_rounds = the rounds the host
                 form needed; HIP events on a stream around the queued launches
  serve_host     mk_session_serve; wall clock around the synchronous call
  composition    what callers wrote before: compute_queue, drain, then the
                 requests that reported MK_ST_CALL_OPEN filtered on the host and
                 queued again, until none is left; wall clock

Every arm is warmed up once, then `repeats` samples are taken with the arms
alternating inside each repeat, and every sample's answers are compared with
the first host serve's.

Prints one JSON line per arm; --out appends them to a file as well."""
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

ARMS = ["serve_device", "serve_host", "composition"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--total", type=int, default=None)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--max-slices", type=int, default=32)
    ap.add_argument("--arms", default=",".join(ARMS))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this probe needs a GPU"
    torch.cuda.init()
    n, total, slices = a.n, a.total or 4 * a.n, a.max_slices
    arms = a.arms.split(",")
    sess = mk.Network(mk.networks.countdown_network()).sessions(n, budget=150)
    plan = sess.plan()
    assert plan.startswith("tier=native"), plan
    stream = torch.cuda.Stream()
    sh = stream.cuda_stream
    rng = np.random.default_rng(0x4D49534B)
    ids = rng.integers(0, n, total).astype(np.uint32)
    x32 = torch.empty(total, dtype=torch.int32, device="cuda")
    mk.generate_inputs_device(total, x32.data_ptr(), seed=0x4D49534B41, gen_kind=1, gen_mask=1023, stream=sh)
    torch.cuda.synchronize()
    d_in = x32.to(torch.int64)
    v = d_in.cpu().numpy()
    d_ids = torch.from_numpy(ids.view(np.int32)).cuda()
    out = torch.empty(total, dtype=torch.int32, device="cuda")
    st = torch.empty(total, dtype=torch.uint8, device="cuda")
    sp = torch.empty(total, dtype=torch.int32, device="cuda")
    left = torch.zeros(2, dtype=torch.int32, device="cuda")

    ref = sess.serve(ids, v, max_slices=slices)
    assert ref.still_open == 0, ref.still_open
    rounds = ref.rounds

    def same(o, s, p):
        return np.array_equal(o, ref.out) and np.array_equal(s, ref.status) and np.array_equal(p, ref.steps)

    def run(arm):
        """One sample: microseconds to serve the whole queue on the reset set."""
        if arm == "serve_device":
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            sess.serve_device(d_ids.data_ptr(), d_in.data_ptr(), total, slices, rounds, out.data_ptr(), st.data_ptr(),
                              sp.data_ptr(), left.data_ptr(), stream=sh)
            e1.record(stream)
            torch.cuda.synchronize()
            assert left.cpu().tolist() == [0, 0]
            assert same(out.cpu().numpy(), st.cpu().numpy(), sp.cpu().numpy().view(np.uint32)), arm
            return e0.elapsed_time(e1) * 1e3, rounds
        t0 = time.perf_counter()
        if arm == "serve_host":
            r = sess.serve(ids, v, max_slices=slices)
            t = (time.perf_counter() - t0) * 1e6
            assert same(r.out, r.status, r.steps) and r.rounds == rounds, arm
            return t, r.rounds
        o, s, p = np.zeros(total, np.int32), np.zeros(total, np.uint8), np.zeros(total, np.uint32)
        todo, passes = np.arange(total), 0
        while todo.size:
            r = sess.compute_queue(ids[todo], v[todo], busy_ok=True)
            o[todo], s[todo], p[todo] = r.out, r.status, r.steps
            # the calls that stayed open: finished by the drain, their answers to their requests
            long = todo[r.status == N.MK_ST_BUDGET]
            if long.size:
                sel = np.sort(ids[long])  # one open call per instance
                d = sess.drain(index=sel, max_slices=slices)
                at = np.searchsorted(sel, ids[long])
                o[long], s[long], p[long] = d.out[at], d.status[at], d.steps[at]
            todo = todo[r.status == N.MK_ST_CALL_OPEN]
            passes += 1
        t = (time.perf_counter() - t0) * 1e6
        assert same(o, s, p), arm
        return t, passes

    samples = {arm: [] for arm in arms}
    launches = {}
    for rep in range(a.repeats + 1):  # the first round warms every arm up
        for arm in arms:
            sess.reset()
            t, launches[arm] = run(arm)
            assert not sess.call_open().any(), arm
            if rep:
                samples[arm].append(t)
    lines = []
    for arm in arms:
        t = samples[arm]
        med = statistics.median(t)
        lines.append({"probe": "sessions_serve", "arm": arm, "n": n, "total": total, "max_slices": slices,
                      "rounds": launches[arm], "us_median": round(med, 1), "us_min": round(min(t), 1),
                      "us_max": round(max(t), 1), "repeats": a.repeats, "samples_us": [round(x, 1) for x in t],
                      "plan": plan})
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
