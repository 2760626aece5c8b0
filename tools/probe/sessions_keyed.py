"""Timing probe for the directory from client keys to instances (DESIGN.md
section 4c, "Client keys").

The example network at n instances (default 1,048,576), device arrays, timed as
tools/probe/sessions_indexed.py does: HIP events on a stream around `span`
back-to-back launches, the arms alternating inside each repeat.  A population
of n/2 keys is bound; a queue holds `total` requests of uniformly random bound
keys.  Arms, for every total given:

  queue         compute_queue_device on the ids the bind gave (the launch a bind feeds)
  bind_hit      bind_device, every key bound
  bind_queue    bind_device chained into compute_queue_device
  churn16       release_device of total/16 bound keys, then bind_device of a
                queue in which one key in 16 is new (as many as were released):
                two queues and two key sets take turns, so every launch pair
                finds the state the one before left
  release_idle  release_device of 65,536 keys none of which is bound (the find,
                the grouping and the padded reset, nothing to free)
  rebind        release_device of 65,536 bound keys, then bind_device of the
                same 65,536 keys, all of them new

A release can only be timed together with what binds its keys again, so
release and the bind of new keys appear as pairs; DESIGN.md takes them apart.
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


def spread(x):
    z = (np.asarray(x).astype(np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize])).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--totals", type=int, nargs="+", default=[1 << 16, 1 << 20])
    ap.add_argument("--release", type=int, default=1 << 16)
    ap.add_argument("--span", type=int, default=200, help="launches per timed span")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--arms", nargs="+", default=None, help="only these arms (for a kernel trace of one of them)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this probe needs a GPU"
    torch.cuda.init()
    n = a.n
    sess = mk.Network(mk.networks.example_network()).sessions(n)
    d = sess.directory()
    rng = np.random.default_rng(64)
    pop = spread(np.arange(n // 2))
    d.bind(pop)
    stream = torch.cuda.Stream()
    sh = stream.cuda_stream
    lines = []
    fresh = n  # spread(fresh ...) have never been keys
    for total in a.totals:
        keys = pop[rng.integers(0, pop.size, total)]
        x = dev(rng.integers(-1000, 1000, total).astype(np.int64))
        d_keys, d_ids = dev(keys), torch.empty(total, dtype=torch.int32, device="cuda")
        out, sp = (torch.empty(total, dtype=torch.int32, device="cuda") for _ in range(2))
        st = torch.empty(total, dtype=torch.uint8, device="cuda")
        # churn16: X[0] and X[1] take turns being bound; X[1] is bound now
        k16 = max(total // 16, 1)
        X = [spread(np.arange(fresh + t * k16, fresh + (t + 1) * k16)) for t in range(2)]
        fresh += 2 * k16
        Q = []
        for t in range(2):
            q = keys.copy()
            q[rng.choice(total, k16, replace=False)] = X[t]
            Q.append(dev(q))
        d_X = [dev(v) for v in X]
        d.bind(X[1])
        turn = [0]
        # rebind / release_idle
        rel = min(a.release, n // 4)
        R = spread(np.arange(fresh, fresh + rel))
        idle = dev(spread(np.arange(fresh + rel, fresh + 2 * rel)))
        fresh += 2 * rel
        d.bind(R)
        d_R, d_rid = dev(R), torch.empty(rel, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

        def queue():
            sess.compute_queue_device(d_ids.data_ptr(), x.data_ptr(), total, out.data_ptr(), st.data_ptr(),
                                      sp.data_ptr(), stream=sh)

        def bind_hit():
            d.bind_device(d_keys.data_ptr(), total, d_ids.data_ptr(), stream=sh)

        def bind_queue():
            bind_hit()
            queue()

        def churn16():
            t = turn[0]
            d.release_device(d_X[1 - t].data_ptr(), k16, stream=sh)
            d.bind_device(Q[t].data_ptr(), total, out.data_ptr(), stream=sh)
            turn[0] = 1 - t

        def release_idle():
            d.release_device(idle.data_ptr(), rel, stream=sh)

        def rebind():
            d.release_device(d_R.data_ptr(), rel, stream=sh)
            d.bind_device(d_R.data_ptr(), rel, d_rid.data_ptr(), stream=sh)

        arms = {"bind_hit": bind_hit, "queue": queue, "bind_queue": bind_queue, "churn16": churn16,
                "release_idle": release_idle, "rebind": rebind}
        if a.arms:
            bind_hit()  # the ids the queue arm runs on
            arms = {k: f for k, f in arms.items() if k in a.arms}
        for f in arms.values():  # warm-up: every arm's code objects and scratch
            for _ in range(10):
                f()
        torch.cuda.synchronize()
        samples = {arm: [] for arm in arms}
        for _ in range(a.repeats):
            for arm, f in arms.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(a.span):
                    f()
                e1.record(stream)
                torch.cuda.synchronize()
                samples[arm].append(e0.elapsed_time(e1) * 1e3 / a.span)
        info = d.info()
        for arm, v in samples.items():
            lines.append({"probe": "sessions_keyed", "arm": arm, "n": n, "total": total,
                          "keys": {"churn16": k16, "release_idle": rel, "rebind": rel}.get(arm, total),
                          "us_per_launch_median": round(statistics.median(v), 3), "us_min": round(min(v), 3),
                          "us_max": round(max(v), 3), "span": a.span, "repeats": a.repeats,
                          "slots": info.slots, "live": info.live, "tombstones": info.tombstones})
        d.release(np.concatenate([X[0], X[1], R]))
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
