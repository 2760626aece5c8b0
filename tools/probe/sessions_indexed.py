"""Timing probe for indexed session launches.

The example network at n instances (default 1,048,576), one call per launch,
device arrays, timed as bench.py's sessions leg does: HIP events on a stream
around `span` back-to-back launches.  Arms:

  plain      mk_session_compute_device on all n
  identity   indexed, sel = 0..n-1
  run16      indexed, m = n/16, a contiguous run that starts mid-block
  stride16   indexed, m = n/16, every 16th session
  random16   indexed, m = n/16, a seeded random increasing list

Every arm is warmed up, then `repeats` samples are taken with the arms
alternating inside each repeat (so drift hits all arms alike); per arm the
median, minimum and maximum of the samples are reported in microseconds per
launch.  mk_session_create (which compiles the session module, now with two
entries) is timed with the host clock, first and later creations apart: the
first one pays the one-time start of the compiler.

Prints one JSON line per arm and one for the creation times; --out appends
them to a file as well."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--span", type=int, default=200, help="launches per timed span")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--creates", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this probe needs a GPU"
    torch.cuda.init()
    n = a.n
    net = mk.Network(mk.networks.example_network())

    created = []
    sess = None
    for _ in range(a.creates):
        if sess is not None:
            sess.close()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sess = net.sessions(n)
        created.append(time.perf_counter() - t0)
    plan = sess.plan()

    stream = torch.cuda.Stream()
    sh = stream.cuda_stream
    m16 = n // 16
    rng = np.random.default_rng(16)
    sels = {
        "identity": np.arange(n, dtype=np.int64),
        "run16": np.arange(m16, dtype=np.int64) + (n // 2 + 100 if n >= 512 else 0),
        "stride16": np.arange(0, n, 16, dtype=np.int64)[:m16],
        "random16": np.sort(rng.choice(n, m16, replace=False)).astype(np.int64),
    }
    x32 = torch.empty(n, dtype=torch.int32, device="cuda")
    mk.generate_inputs_device(n, x32.data_ptr(), seed=0x4D49534B41, stream=sh)
    torch.cuda.synchronize()
    x = x32.to(torch.int64)
    out = torch.empty(n, dtype=torch.int32, device="cuda")
    st = torch.empty(n, dtype=torch.uint8, device="cuda")
    sp = torch.empty(n, dtype=torch.int32, device="cuda")
    d_sel = {k: torch.from_numpy(v.astype(np.uint32).view(np.int32)).cuda() for k, v in sels.items()}
    torch.cuda.synchronize()

    def launch(arm):
        if arm == "plain":
            sess.compute_device(x.data_ptr(), out.data_ptr(), st.data_ptr(), sp.data_ptr(), stream=sh)
        else:
            s = d_sel[arm]
            sess.compute_device(x.data_ptr(), out.data_ptr(), st.data_ptr(), sp.data_ptr(), stream=sh,
                                index_ptr=s.data_ptr(), m=s.numel())

    arms = ["plain"] + list(sels)
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
    for arm in arms:
        v = samples[arm]
        lines.append({"probe": "sessions_indexed", "arm": arm, "n": n, "m": n if arm in ("plain", "identity") else m16,
                      "us_per_launch_median": round(statistics.median(v), 3), "us_min": round(min(v), 3),
                      "us_max": round(max(v), 3), "span": a.span, "repeats": a.repeats})
    lines.append({"probe": "sessions_indexed", "arm": "create", "n": n, "first_s": round(created[0], 3),
                  "later_s": [round(t, 3) for t in created[1:]], "plan": plan})
    for ln in lines:
        print(json.dumps(ln))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
