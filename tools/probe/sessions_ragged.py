"""Timing probe for ragged session bursts.

The example network at n instances (default 1,048,576), device arrays, timed
as the other session probes are: HIP events on a stream around `span`
back-to-back launches.  Arms:

  indexed1   mk_session_compute_indexed_device, sel = 0..n-1, one call each
  ragged1    mk_session_compute_ragged_device, the same list, every count 1
  ragged     ragged on a seeded random increasing list of m (default 65,536)
             sessions; counts 1 + G with G geometric on 0, 1, 2, ... of mean 2,
             capped at 16
  shrinking  the same calls done without ragged launches: max(count) indexed
             launches, launch k on the entries with count > k (one timed unit
             is the whole series)

Every arm is warmed up, then `repeats` samples are taken with the arms
alternating inside each repeat.  Per arm: median, minimum and maximum in
microseconds per unit, the calls a unit makes, and nanoseconds per call.

Prints one JSON line per arm; --out appends them to a file as well."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import misaka_net_amd as mk  # noqa: E402


def dev_u32(a):
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.uint32).view(np.int32)).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--m", type=int, default=1 << 16, help="listed sessions of the ragged and shrinking arms")
    ap.add_argument("--span", type=int, default=200, help="units per timed span")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this probe needs a GPU"
    torch.cuda.init()
    n, m = a.n, min(a.m, a.n)
    sess = mk.Network(mk.networks.example_network()).sessions(n)
    plan = sess.plan()
    stream = torch.cuda.Stream()
    sh = stream.cuda_stream

    rng = np.random.default_rng(65536)
    sel = np.sort(rng.choice(n, m, replace=False)).astype(np.int64)
    cnt = np.minimum(rng.geometric(1.0 / 3.0, m), 16).astype(np.int64)  # 1 + (geometric - 1): mean 3 before the cap
    off = np.zeros(m + 1, np.int64)
    np.cumsum(cnt, out=off[1:])
    total = int(off[-1])
    size = max(n, total)

    x32 = torch.empty(size, dtype=torch.int32, device="cuda")
    mk.generate_inputs_device(size, x32.data_ptr(), seed=0x4D49534B41, stream=sh)
    torch.cuda.synchronize()
    x = x32.to(torch.int64)
    out = torch.empty(size, dtype=torch.int32, device="cuda")
    st = torch.empty(size, dtype=torch.uint8, device="cuda")
    sp = torch.empty(size, dtype=torch.int32, device="cuda")
    io = (out.data_ptr(), st.data_ptr(), sp.data_ptr())
    d_all, d_ones = dev_u32(np.arange(n)), dev_u32(np.arange(n + 1))
    d_sel, d_off = dev_u32(sel), dev_u32(off)
    shrink = [dev_u32(sel[cnt > k]) for k in range(int(cnt.max()))]  # launch k of the shrinking series
    torch.cuda.synchronize()

    def launch(arm):
        if arm == "indexed1":
            sess.compute_device(x.data_ptr(), *io, stream=sh, index_ptr=d_all.data_ptr(), m=n)
        elif arm == "ragged1":
            sess.compute_ragged_device(x.data_ptr(), d_ones.data_ptr(), n, *io, stream=sh, index_ptr=d_all.data_ptr(),
                                       m=n)
        elif arm == "ragged":
            sess.compute_ragged_device(x.data_ptr(), d_off.data_ptr(), total, *io, stream=sh,
                                       index_ptr=d_sel.data_ptr(), m=m)
        else:
            for s in shrink:
                sess.compute_device(x.data_ptr(), *io, stream=sh, index_ptr=s.data_ptr(), m=s.numel())

    arms = {"indexed1": (n, 1), "ragged1": (n, 1), "ragged": (total, 1), "shrinking": (total, len(shrink))}
    for arm in arms:  # warm-up: every arm's code objects and buffers
        for _ in range(20):
            launch(arm)
    torch.cuda.synchronize()
    samples = {arm: [] for arm in arms}
    for _ in range(a.repeats):
        for arm in arms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(a.span):
                launch(arm)
            e1.record(stream)
            torch.cuda.synchronize()
            samples[arm].append(e0.elapsed_time(e1) * 1e3 / a.span)
    sess.close()

    lines = []
    for arm, (calls, launches) in arms.items():
        v = samples[arm]
        med = statistics.median(v)
        lines.append({"probe": "sessions_ragged", "arm": arm, "n": n, "m": n if calls == n else m, "calls": calls,
                      "launches_per_unit": launches, "max_count": int(cnt.max()), "us_per_unit_median": round(med, 3),
                      "us_min": round(min(v), 3), "us_max": round(max(v), 3),
                      "ns_per_call_median": round(med * 1e3 / calls, 4), "span": a.span, "repeats": a.repeats,
                      "plan": plan})
    for ln in lines:
        print(json.dumps(ln))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
