"""Timing probe for session snapshots.

The example network at n instances (default 1,048,576) after two calls,
device arrays, timed as bench.py's sessions leg does: HIP events on a stream
around `span` back-to-back launches.  Arms:

  snapshot_all   mk_session_snapshot_device of all n
  restore_all    mk_session_restore_device of all n from that block
  snapshot_sel   ... of a seeded random increasing list of m (default 65,536)
  restore_sel    ... of that list, from the list's own block

Every arm is warmed up, then `repeats` samples are taken with the arms
alternating inside each repeat (so drift hits all arms alike); per arm the
median, minimum and maximum of the samples are reported in microseconds per
launch, and the bytes moved per second against the float4-copy ceiling of
6.29 TB/s, by the byte model written out where the lines are made.

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

CEILING = 6.29e12  # bytes/s, a float4 copy kernel on this part


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
    sess = mk.Network(mk.networks.example_network()).sessions(n)
    plan = sess.plan()
    lay = sess.layout()

    stream = torch.cuda.Stream()
    sh = stream.cuda_stream
    x32 = torch.empty(n, dtype=torch.int32, device="cuda")
    mk.generate_inputs_device(n, x32.data_ptr(), seed=0x4D49534B41, stream=sh)
    torch.cuda.synchronize()
    x = x32.to(torch.int64)
    out = torch.empty(n, dtype=torch.int32, device="cuda")
    st = torch.empty(n, dtype=torch.uint8, device="cuda")
    for _ in range(2):  # a state that is not the post-reset one
        sess.compute_device(x.data_ptr(), out.data_ptr(), st.data_ptr(), None, stream=sh)
    sel = np.sort(np.random.default_rng(16).choice(n, m, replace=False)).astype(np.uint32)
    d_sel = torch.from_numpy(sel.view(np.int32)).cuda()
    rec_all = torch.zeros(lay.rows * n, dtype=torch.int32, device="cuda")
    rec_sel = torch.zeros(lay.rows * m, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def launch(arm):
        if arm == "snapshot_all":
            sess.snapshot_device(rec_all.data_ptr(), stream=sh)
        elif arm == "restore_all":
            sess.restore_device(lay, rec_all.data_ptr(), n, stream=sh)
        elif arm == "snapshot_sel":
            sess.snapshot_device(rec_sel.data_ptr(), stream=sh, index_ptr=d_sel.data_ptr(), m=m)
        else:
            sess.restore_device(lay, rec_sel.data_ptr(), m, stream=sh, index_ptr=d_sel.data_ptr(), m=m)

    arms = ["snapshot_all", "restore_all", "snapshot_sel", "restore_sel"]
    for arm in arms:  # warm-up; the snapshots come first, so the restores have their blocks
        for _ in range(20):
            launch(arm)
    torch.cuda.synchronize()
    held = int((rec_all.view(lay.rows, n)[0] == 1).sum().item())
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
    # the set still computes: a call after the last restore, against the state the snapshot was taken at
    sess.compute_device(x.data_ptr(), out.data_ptr(), st.data_ptr(), None, stream=sh)
    torch.cuda.synchronize()
    assert int((st == 0x10).sum().item()) == n, "a call after the restores did not answer everywhere"
    sess.close()

    # bytes per entry (every session here is held by the tier of the set): a snapshot writes the record
    # and reads the holder's state; a native restore reads held, the ips, the depths and the native
    # section, writes the native state and zeroes the interpreter's words but the stack entries; a
    # canonical restore reads and writes the canonical part with the stack entries below the depths,
    # none in this state's case on the example network
    rec_b = lay.rows * 4
    canon_b = (lay.rows - lay.native_rows) * 4
    words_b = canon_b - lay.nstack * lay.stack_cap * 4
    native_b = lay.native_rows * 4
    checks_b = (1 + lay.nprog + lay.nstack) * 4
    per_arm = {"snapshot": rec_b + (native_b if native_b else words_b),
               "restore": checks_b + 2 * native_b + words_b if native_b else 2 * words_b}
    lines = []
    for arm in arms:
        v = samples[arm]
        k = n if arm.endswith("_all") else m
        per = per_arm[arm.split("_")[0]]
        med = statistics.median(v)
        bps = per * k / (med * 1e-6)
        lines.append({"probe": "sessions_snapshot", "arm": arm, "n": n, "m": k, "rows": lay.rows,
                      "native_rows": lay.native_rows, "held": held, "us_per_launch_median": round(med, 3),
                      "us_min": round(min(v), 3), "us_max": round(max(v), 3), "bytes_per_entry": per,
                      "tb_per_s": round(bps / 1e12, 3), "of_ceiling": round(bps / CEILING, 3), "span": a.span,
                      "repeats": a.repeats, "samples_us": [round(t, 3) for t in v], "plan": plan})
    for ln in lines:
        print(json.dumps(ln))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
