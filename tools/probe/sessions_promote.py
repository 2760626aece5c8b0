"""Timing probe for session promotion.

The countdown network at n instances (default 1,048,576), budget 1000.  One
call with inputs up to 1023 hands most instances to the interpreter; resumes
close every call.  That DEGRADED state is snapshotted, promoted, and the
PROMOTED state snapshotted too; restoring one block or the other puts the set
into either state.  Device arrays, timed as bench.py's sessions leg does: HIP
events on a stream around `span` back-to-back launches.  Arms:

  call_degraded   one call (inputs up to 63: none can hand off) on the degraded set
  call_promoted   ... on the promoted set
  call_fresh      ... on a second set that never handed anything off
  call_restored   ... on the first set again, holding the second set's state (a
                  native restore of its snapshot): the promoted set's
                  allocation with the fresh set's state
  restore_all     mk_session_restore_device of the degraded block, all n
  cycle_all       that restore, then mk_session_promote_device of all n
  restore_sel     ... of a seeded random increasing list of m (default 65,536)
  cycle_sel       ... then the promotion of that list

A promotion needs interpreter-held instances to work on, so it is timed
behind the restore that provides them; promote_* = cycle_* - restore_* is
reported as a derived line from the medians.  Every arm is warmed up, then
`repeats` samples are taken with the arms alternating inside each repeat.

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--m", type=int, default=1 << 16)
    ap.add_argument("--span", type=int, default=200, help="launches per timed span")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this probe needs a GPU"
    torch.cuda.init()
    n, m = a.n, min(a.m, a.n)
    net = mk.Network(mk.networks.countdown_network())
    sess, fresh = net.sessions(n, budget=1000), net.sessions(n, budget=1000)
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
    out = torch.empty(n, dtype=torch.int32, device="cuda")
    st = torch.empty(n, dtype=torch.uint8, device="cuda")
    sess.compute_device(big.data_ptr(), out.data_ptr(), st.data_ptr(), None, stream=sh)
    torch.cuda.synchronize()
    for _ in range(64):
        if not sess.call_open().any():
            break
        sess.resume(steps=False)
    assert not sess.call_open().any()
    rec_deg = torch.zeros(lay.rows * n, dtype=torch.int32, device="cuda")
    rec_pro = torch.zeros(lay.rows * n, dtype=torch.int32, device="cuda")
    flags = torch.zeros(n, dtype=torch.uint8, device="cuda")
    sess.snapshot_device(rec_deg.data_ptr(), stream=sh)
    sess.promote_device(flags.data_ptr(), stream=sh)
    sess.snapshot_device(rec_pro.data_ptr(), stream=sh)
    rec_new = torch.zeros(lay.rows * n, dtype=torch.int32, device="cuda")
    fresh.snapshot_device(rec_new.data_ptr(), stream=sh)
    torch.cuda.synchronize()
    degraded = n - int((rec_deg.view(lay.rows, n)[0] == 1).sum().item())
    promoted = int(flags.sum().item())
    assert promoted == degraded and int((rec_pro.view(lay.rows, n)[0] == 1).sum().item()) == n
    sel = np.sort(np.random.default_rng(16).choice(n, m, replace=False)).astype(np.uint32)
    d_sel = torch.from_numpy(sel.view(np.int32)).cuda()
    rec_sel = rec_deg.view(lay.rows, n)[:, torch.from_numpy(sel.astype(np.int64)).cuda()].contiguous()
    held_sel = m - int((rec_sel[0] == 1).sum().item())
    torch.cuda.synchronize()

    def call(s):
        s.compute_device(small.data_ptr(), out.data_ptr(), st.data_ptr(), None, stream=sh)

    def prepare(arm):
        if arm == "call_degraded":
            sess.restore_device(lay, rec_deg.data_ptr(), n, stream=sh)
        elif arm == "call_promoted":
            sess.restore_device(lay, rec_pro.data_ptr(), n, stream=sh)
        elif arm == "call_restored":
            sess.restore_device(lay, rec_new.data_ptr(), n, stream=sh)

    def launch(arm):
        if arm == "call_fresh":
            call(fresh)
        elif arm.startswith("call_"):
            call(sess)
        elif arm.endswith("_all"):
            sess.restore_device(lay, rec_deg.data_ptr(), n, stream=sh)
            if arm == "cycle_all":
                sess.promote_device(flags.data_ptr(), stream=sh)
        else:
            sess.restore_device(lay, rec_sel.data_ptr(), m, stream=sh, index_ptr=d_sel.data_ptr(), m=m)
            if arm == "cycle_sel":
                sess.promote_device(flags.data_ptr(), stream=sh, index_ptr=d_sel.data_ptr(), m=m)

    arms = ["call_degraded", "call_promoted", "call_fresh", "call_restored", "restore_all", "cycle_all",
            "restore_sel", "cycle_sel"]
    for arm in arms:
        prepare(arm)
        for _ in range(20):
            launch(arm)
    torch.cuda.synchronize()
    samples = {arm: [] for arm in arms}
    for _ in range(a.repeats):
        for arm in arms:
            prepare(arm)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(a.span):
                launch(arm)
            e1.record(stream)
            torch.cuda.synchronize()
            samples[arm].append(e0.elapsed_time(e1) * 1e3 / a.span)
    # both sets still compute, and agree: the promoted set against the one that never handed off
    got = {}
    for name, s in (("promoted", sess), ("fresh", fresh)):
        if name == "promoted":
            sess.restore_device(lay, rec_pro.data_ptr(), n, stream=sh)
        call(s)
        torch.cuda.synchronize()
        got[name] = (out.clone(), st.clone())
    assert torch.equal(got["promoted"][0], got["fresh"][0]) and torch.equal(got["promoted"][1], got["fresh"][1])
    sess.close()
    fresh.close()

    lines = []
    med = {}
    for arm in arms:
        v = samples[arm]
        med[arm] = statistics.median(v)
        lines.append({"probe": "sessions_promote", "arm": arm, "n": n, "m": m if arm.endswith("_sel") else n,
                      "degraded": held_sel if arm.endswith("_sel") else degraded, "rows": lay.rows,
                      "us_per_launch_median": round(med[arm], 3), "us_min": round(min(v), 3),
                      "us_max": round(max(v), 3), "span": a.span, "repeats": a.repeats,
                      "samples_us": [round(t, 3) for t in v], "plan": plan})
    for k in ("all", "sel"):
        lines.append({"probe": "sessions_promote", "arm": f"promote_{k}", "derived": f"cycle_{k} - restore_{k}, medians",
                      "n": n, "m": m if k == "sel" else n, "degraded": held_sel if k == "sel" else degraded,
                      "us_per_launch_median": round(med[f"cycle_{k}"] - med[f"restore_{k}"], 3)})
    for ln in lines:
        print(json.dumps(ln))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
