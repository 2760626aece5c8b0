"""Timing probe for request queues.

The example network at n instances (default 1,048,576) and the calls of
tools/probe/sessions_ragged.py: a seeded random list of m (default 65,536)
sessions, counts 1 + G with G geometric of mean 2, capped at 16 -- 195,644
calls.  The queue is those calls as (session, value) requests in a seeded
random arrival order.  Device arms, HIP events on a stream around `span`
back-to-back units:

  ragged       mk_session_compute_ragged_device on inputs grouped beforehand:
               the floor
  queue        mk_session_compute_queue_device on the requests in arrival order
  group        mk_requests_group_device alone
  ragged_K, queue_K, group_K
               the same on the first K requests of the queue, K = 1000, 2000
  queue_K_tiled, group_K_tiled
               queue_K and group_K with the one-block path for queues of one
               tile switched off (MK_GROUP_ONE_TILE=0)

Host arms, wall time around `host_span` units, host arrays in and out:

  host_numpy   numpy stable argsort, unique, compute_ragged, un-permute
  host_group   the numpy part of host_numpy alone (no launch)
  host_queue   compute_queue
  host_numpy_K, host_group_K, host_queue_K
               the same on the first K requests, 40 x `host_span` units a span

--trace ARM runs one device arm alone, `span` units and nothing else, for
`rocprofv3 --kernel-trace --stats -- python tools/probe/sessions_queue.py
--trace queue`.

Every arm is warmed up, then `repeats` samples are taken with the arms
alternating inside each repeat.  Per arm: median, minimum and maximum in
microseconds per unit.  Prints one JSON line per arm; --out appends them to
a file as well."""
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


def dev_u32(a):
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.uint32).view(np.int32)).cuda()


def grouped(ids):
    perm = np.argsort(ids, kind="stable")
    sel, cnt = np.unique(ids, return_counts=True)
    off = np.zeros(sel.size + 1, np.int64)
    np.cumsum(cnt, out=off[1:])
    return perm, sel, cnt, off


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--m", type=int, default=1 << 16, help="sessions with requests")
    ap.add_argument("--span", type=int, default=200, help="units per timed span of a device arm")
    ap.add_argument("--host-span", type=int, default=5, help="units per timed span of a host arm")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--small", type=int, nargs="*", default=[1000, 2000])
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", default=None, metavar="ARM",
                    help="run only this device arm, `span` units, for a kernel trace taken around the probe")
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
    cnt = np.minimum(rng.geometric(1.0 / 3.0, m), 16).astype(np.int64)
    total = int(cnt.sum())
    queue = rng.permutation(np.repeat(sel, cnt))  # arrival order

    x32 = torch.empty(total, dtype=torch.int32, device="cuda")
    mk.generate_inputs_device(total, x32.data_ptr(), seed=0x4D49534B41, stream=sh)
    torch.cuda.synchronize()
    x = x32.to(torch.int64)
    h_x = x.cpu().numpy()
    out = torch.empty(total, dtype=torch.int32, device="cuda")
    st = torch.empty(total, dtype=torch.uint8, device="cuda")
    sp = torch.empty(total, dtype=torch.int32, device="cuda")
    io = (out.data_ptr(), st.data_ptr(), sp.data_ptr())

    sizes = [total] + [k for k in a.small if k < total]
    dev = {}
    for k in sizes:
        ids = queue[:k]
        perm, s, c, off = grouped(ids)
        M = min(k, n)
        nb = mk.network.group_requests_tmp_bytes(n, k)
        dev[k] = dict(ids=dev_u32(ids), sel=dev_u32(s), off=dev_u32(off), m=s.size,
                      g=[torch.empty(w, dtype=torch.int32, device="cuda") for w in (k, M, M + 1, 1)],
                      tmp=torch.empty(nb, dtype=torch.uint8, device="cuda"), nb=nb)
    torch.cuda.synchronize()

    def device_arm(kind, k):
        d = dev[k]
        if kind == "ragged":
            return lambda: sess.compute_ragged_device(x.data_ptr(), d["off"].data_ptr(), k, *io, stream=sh,
                                                      index_ptr=d["sel"].data_ptr(), m=d["m"])
        if kind == "queue":
            return lambda: sess.compute_queue_device(d["ids"].data_ptr(), x.data_ptr(), k, *io, stream=sh)
        return lambda: mk.network.group_requests_device(n, d["ids"].data_ptr(), k, *(t.data_ptr() for t in d["g"]),
                                                        d["tmp"].data_ptr(), d["nb"], stream=sh)

    def host_group(k):
        perm, s, c, off = grouped(queue[:k])
        return perm, s, c, h_x[:k][perm]

    def host_numpy(k=total):
        perm, s, c, v = host_group(k)
        r = sess.compute_ragged(v, c, index=s)
        o, t, p = np.empty_like(r.out), np.empty_like(r.status), np.empty_like(r.steps)
        o[perm], t[perm], p[perm] = r.out, r.status, r.steps
        return o, t, p

    stand_in = (np.zeros(total, np.int32), np.zeros(total, np.uint8), np.zeros(total, np.uint32))

    def host_group_only(k=total):
        perm, s, c, v = host_group(k)
        o, t, p = np.empty(k, np.int32), np.empty(k, np.uint8), np.empty(k, np.uint32)
        o[perm], t[perm], p[perm] = (z[:k] for z in stand_in)  # the un-permute's cost, on stand-in results

    arms = {}
    for k in sizes:
        tag = "" if k == total else f"_{k}"
        for kind in ("ragged", "queue", "group"):
            arms[kind + tag] = (device_arm(kind, k), k, True)
    # one-tile queues through the kernels of the larger ones (MK_GROUP_ONE_TILE is read at every launch)
    def tiled(fn):
        def run():
            os.environ["MK_GROUP_ONE_TILE"] = "0"
            fn()
            del os.environ["MK_GROUP_ONE_TILE"]
        return run

    for k in sizes[1:]:
        if k <= 2048:
            for kind in ("queue", "group"):
                arms[f"{kind}_{k}_tiled"] = (tiled(device_arm(kind, k)), k, True)
    arms["host_numpy"] = (host_numpy, total, False)
    arms["host_group"] = (host_group_only, total, False)
    arms["host_queue"] = (lambda: sess.compute_queue(queue, h_x), total, False)
    for k in sizes[1:]:
        arms[f"host_numpy_{k}"] = (lambda k=k: host_numpy(k), k, False)
        arms[f"host_group_{k}"] = (lambda k=k: host_group_only(k), k, False)
        arms[f"host_queue_{k}"] = (lambda k=k: sess.compute_queue(queue[:k], h_x[:k]), k, False)

    if a.trace:
        for _ in range(a.span):
            arms[a.trace][0]()
        torch.cuda.synchronize()
        sess.close()
        return

    # the two host forms agree before anything is timed
    # (from the same state: a session's second call need not take the steps of its first)
    r0 = host_numpy()
    sess.reset()
    r1 = sess.compute_queue(queue, h_x)
    diff = [int((x != y).sum()) for x, y in zip(r0, (r1.out, r1.status, r1.steps))]
    assert diff == [0, 0, 0], f"out / status / steps differ at {diff} of {total} requests"

    for arm, (fn, _, on_device) in arms.items():  # warm-up: every arm's code objects and buffers
        for _ in range(20 if on_device else 2):
            fn()
    torch.cuda.synchronize()
    samples = {arm: [] for arm in arms}

    def hspan(arm):  # units per span of a host arm: more for the small queues
        return a.host_span if arms[arm][1] == total else a.host_span * 40
    for _ in range(a.repeats):
        for arm, (fn, _, on_device) in arms.items():
            if on_device:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(a.span):
                    fn()
                e1.record(stream)
                torch.cuda.synchronize()
                samples[arm].append(e0.elapsed_time(e1) * 1e3 / a.span)
            else:
                t0 = time.perf_counter()
                for _ in range(hspan(arm)):
                    fn()
                samples[arm].append((time.perf_counter() - t0) * 1e6 / hspan(arm))
    sess.close()

    lines = []
    for arm, (_, k, on_device) in arms.items():
        v = samples[arm]
        med = statistics.median(v)
        lines.append({"probe": "sessions_queue", "arm": arm, "n": n, "requests": k,
                      "sessions": int(np.unique(queue[:k]).size), "clock": "hip_events" if on_device else "wall",
                      "us_per_unit_median": round(med, 3), "us_min": round(min(v), 3), "us_max": round(max(v), 3),
                      "ns_per_request_median": round(med * 1e3 / k, 4),
                      "span": a.span if on_device else hspan(arm), "repeats": a.repeats, "plan": plan})
    for ln in lines:
        print(json.dumps(ln))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
