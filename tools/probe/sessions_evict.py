"""Timing probe for use stamps, idle selection and eviction on a tracked
directory ("Idle clients"); a sibling of
tools/probe/sessions_keyed.py at the same shape and timed the same way: the
example network at n instances (default 1,048,576), n/2 keys bound, device
arrays, HIP events on a stream around `span` back-to-back launches, the arms
alternating inside each repeat.  Two sets, one with an untracked and one with a
tracked directory.  Arms, for every total given:

  bind_hit            bind_device on the untracked directory, every key bound
  bind_hit_tracked    the same on the tracked one: the cost of the stamp
  bind_evict_idle     bind_evict_device, every key bound, max_evict total/16:
                      nothing to evict, the fixed cost of the extra launches
  idle_select         idle_device of 65,536 on the half-full directory

and then, with the tracked directory filled to the last instance:

  evict16             bind_evict_device of a queue in which one key in 16 has
                      never been seen, max_evict total/16: the clients silent
                      longest make room.  The new keys are written into the
                      queue on the stream before every launch (two small
                      PyTorch kernels inside the timed span).  Compare churn16
                      of sessions_keyed.py, where the host lists the keys.

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
from sessions_keyed import dev, spread  # noqa: E402


def timed(arms, stream, span, repeats):
    for f in arms.values():  # warm-up: every arm's code objects and scratch
        for _ in range(10):
            f()
    torch.cuda.synchronize()
    samples = {arm: [] for arm in arms}
    for _ in range(repeats):
        for arm, f in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(span):
                f()
            e1.record(stream)
            torch.cuda.synchronize()
            samples[arm].append(e0.elapsed_time(e1) * 1e3 / span)
    return samples


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--totals", type=int, nargs="+", default=[1 << 16, 1 << 20])
    ap.add_argument("--select", type=int, default=1 << 16)
    ap.add_argument("--span", type=int, default=200, help="launches per timed span")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--arms", nargs="+", default=None, help="only these arms")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this probe needs a GPU"
    torch.cuda.init()
    n = a.n
    net = mk.Network(mk.networks.example_network())
    plain, tracked = net.sessions(n), net.sessions(n)
    d, t = plain.directory(), tracked.directory()
    t.track()
    rng = np.random.default_rng(64)
    pop = spread(np.arange(n // 2))
    d.bind(pop)
    # the tracked population in 16 binds, so that there are 16 ages to select among
    for part in np.array_split(pop, 16):
        t.bind(part)
    stream = torch.cuda.Stream()
    sh = stream.cuda_stream
    lines = []

    def report(samples, total, keys, info, extra=None):
        for arm, v in samples.items():
            ln = {"probe": "sessions_evict", "arm": arm, "n": n, "total": total, "keys": keys.get(arm, total),
                  "us_per_launch_median": round(statistics.median(v), 3), "us_min": round(min(v), 3),
                  "us_max": round(max(v), 3), "span": a.span, "repeats": a.repeats, "slots": info.slots,
                  "live": info.live, "tombstones": info.tombstones}
            ln.update(extra or {})
            lines.append(ln)

    want = lambda arms: {k: f for k, f in arms.items() if not a.arms or k in a.arms}  # noqa: E731
    sel = min(a.select, n)
    sel_k = torch.empty(sel, dtype=torch.int64, device="cuda")
    sel_i, sel_c = torch.empty(sel, dtype=torch.int32, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda")
    for total in a.totals:
        keys = pop[rng.integers(0, pop.size, total)]
        d_keys, d_ids = dev(keys), torch.empty(total, dtype=torch.int32, device="cuda")
        k16 = max(total // 16, 1)
        cnt = torch.empty(4, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        arms = want({
            "bind_hit": lambda: d.bind_device(d_keys.data_ptr(), total, d_ids.data_ptr(), stream=sh),
            "bind_hit_tracked": lambda: t.bind_device(d_keys.data_ptr(), total, d_ids.data_ptr(), stream=sh),
            "bind_evict_idle": lambda: t.bind_evict_device(d_keys.data_ptr(), total, d_ids.data_ptr(), k16,
                                                           counts_ptr=cnt.data_ptr(), stream=sh),
            "idle_select": lambda: t.idle_device(sel, sel_k.data_ptr(), sel_i.data_ptr(), sel_c.data_ptr(),
                                                 stream=sh),
        })
        if arms:
            report(timed(arms, stream, a.span, a.repeats), total, {"idle_select": sel}, t.info(),
                   {"selected": int(sel_c.cpu().numpy().view(np.uint32)[0])} if "idle_select" in arms else None)
    if not a.arms or "evict16" in a.arms:
        # fill the tracked directory, again in 16 binds
        for part in np.array_split(spread(np.arange(n // 2, n)), 16):
            t.bind(part)
        assert t.info().free == 0
        for total in a.totals:
            k16 = max(total // 16, 1)
            q = dev(pop[rng.integers(0, pop.size, total)])
            at = torch.from_numpy(rng.choice(total, k16, replace=False)).cuda()
            step = torch.arange(k16, dtype=torch.int64, device="cuda")
            d_ids, cnt = torch.empty(total, dtype=torch.int32, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")
            turn = [0]
            torch.cuda.synchronize()

            def evict16():
                # keys that no queue has held: 2^62 + a counter (any value is a key)
                turn[0] += 1
                with torch.cuda.stream(stream):
                    q[at] = step + ((1 << 62) + total * (1 << 24) + turn[0] * k16)
                t.bind_evict_device(q.data_ptr(), total, d_ids.data_ptr(), k16, counts_ptr=cnt.data_ptr(), stream=sh)

            report(timed({"evict16": evict16}, stream, a.span, a.repeats), total, {"evict16": k16}, t.info(),
                   {"last_counts": cnt.cpu().numpy().view(np.uint32).tolist()})
    plain.close()
    tracked.close()
    for ln in lines:
        print(json.dumps(ln))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
