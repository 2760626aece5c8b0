"""Timing probe for the host forms of a session set:
host arrays in, host arrays out, every call ending in its own synchronise.

The example network at n = 1 and n = 4096 instances (--n), one arm per form:

  seq      compute_seq, 2 calls per instance
  indexed  compute on every second instance (the only one for n = 1)
  ragged   compute_ragged, entry t making 1 + t % 3 calls
  queue    compute_queue, the ragged arm's calls in a seeded arrival order

Wall time around `span` back-to-back calls.  Every arm is warmed up, then
`repeats` samples are taken with the arms alternating inside each repeat.
Per arm: median, minimum and maximum in microseconds per call.  Prints one
JSON line per arm; --out appends them to a file as well.  To compare two
builds of the library run the probe once per build, the builds taking turns
(tools/probe/lib_ab.sh)."""
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
    ap.add_argument("--n", type=int, nargs="*", default=[1, 4096])
    ap.add_argument("--span", type=int, default=100, help="calls per timed span")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--label", default=None, help="copied into every line (which build this is)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this probe needs a GPU"
    torch.cuda.init()
    net = mk.Network(mk.networks.example_network())
    arms, sets = {}, []
    for n in a.n:
        sess = net.sessions(n)
        sets.append(sess)
        rng = np.random.default_rng(n)
        cnt = 1 + np.arange(n) % 3
        total = int(cnt.sum())
        x = rng.integers(-1000, 1000, max(2 * n, total)).astype(np.int64)
        sel = np.arange(0, n, 2)
        ids = rng.permutation(np.repeat(np.arange(n), cnt))
        arms[f"seq_{n}"] = (lambda s=sess, v=x[:2 * n].reshape(2, n): s.compute_seq(v), n, 2 * n)
        arms[f"indexed_{n}"] = (lambda s=sess, v=x[:sel.size], i=sel: s.compute(v, index=i), n, sel.size)
        arms[f"ragged_{n}"] = (lambda s=sess, v=x[:total], c=cnt: s.compute_ragged(v, c), n, total)
        arms[f"queue_{n}"] = (lambda s=sess, v=x[:total], i=ids: s.compute_queue(i, v), n, total)
    plan = sets[0].plan()

    for fn, _, _ in arms.values():  # warm-up: code objects, the staging, the queue scratch
        for _ in range(20):
            fn()
    samples = {arm: [] for arm in arms}
    for _ in range(a.repeats):
        for arm, (fn, _, _) in arms.items():
            t0 = time.perf_counter()
            for _ in range(a.span):
                fn()
            samples[arm].append((time.perf_counter() - t0) * 1e6 / a.span)
    for s in sets:
        s.close()

    lines = []
    for arm, (_, n, calls) in arms.items():
        v = samples[arm]
        lines.append({"probe": "sessions_host", "arm": arm, "n": n, "calls": calls, "clock": "wall",
                      "us_per_unit_median": round(statistics.median(v), 3), "us_min": round(min(v), 3),
                      "us_max": round(max(v), 3), "span": a.span, "repeats": a.repeats, "plan": plan})
        if a.label:
            lines[-1]["label"] = a.label
    for ln in lines:
        print(json.dumps(ln))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
