"""One call of every form of a session set at n = 600, for a trace of the GPU
work each issues:

  rocprofv3 --kernel-trace --memory-copy-trace --output-format json -d DIR -o t -- \
      python tools/probe/sessions_forms_trace.py
  python tools/probe/sessions_forms_trace.py --fold DIR > list.txt

The four host forms (seq, indexed, ragged, queue), their device forms, a
snapshot and a restore (host and device), each followed by a synchronise, so
the order of the trace is the order of the calls.  --fold prints the ordered
list of kernel names and of copies with direction and bytes: two builds of the
library issue the same GPU work when their lists are equal.  The small copies
through pinned memory are done by the runtime's blit kernels and appear as
`__amd_rocclr_copyBuffer` (a memset as `__amd_rocclr_fillBufferAligned`), one
line per copy, without a size; only the large copies are copy records."""
import glob
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

NS = 600


def fold(d):
    paths = sorted(glob.glob(os.path.join(d, "**", "*_results.json"), recursive=True))
    assert paths, f"no rocprofv3 json under {d}"
    for p in paths:
        with open(p) as f:
            t = json.load(f)["rocprofiler-sdk-tool"][0]
        names = {k["kernel_id"]: k.get("formatted_kernel_name") or k["kernel_name"] for k in t["kernel_symbols"]}
        ops = {}
        for k in t["strings"]["buffer_records"]:
            if "MEMORY_COPY" in k["kind"]:
                ops = dict(enumerate(k["operations"]))
        ev = [(r["start_timestamp"], "kernel " + names[r["dispatch_info"]["kernel_id"]])
              for r in t["buffer_records"]["kernel_dispatch"]]
        ev += [(r["start_timestamp"], f"copy {ops.get(r['operation'], r['operation'])} {r['bytes']}")
               for r in t["buffer_records"]["memory_copy"]]
        for _, what in sorted(ev):
            print(what)


def main():
    import torch

    import misaka_net_amd as mk

    torch.cuda.init()
    s = mk.Network(mk.networks.example_network()).sessions(NS)
    stream = torch.cuda.Stream()
    sh = stream.cuda_stream
    rng = np.random.default_rng(NS)
    sel = np.sort(rng.choice(NS, 257, replace=False))
    cnt = 1 + np.arange(sel.size) % 3
    total = int(cnt.sum())
    off = np.zeros(sel.size + 1, np.int64)
    np.cumsum(cnt, out=off[1:])
    ids = rng.permutation(np.repeat(sel, cnt))
    x = rng.integers(-1000, 1000, 2 * NS).astype(np.int64)

    def u32(a):
        return torch.from_numpy(np.ascontiguousarray(a).astype(np.uint32).view(np.int32)).cuda()

    d_x, d_sel, d_off, d_ids = torch.from_numpy(x).cuda(), u32(sel), u32(off), u32(ids)
    out = torch.empty(2 * NS, dtype=torch.int32, device="cuda")
    st = torch.empty(2 * NS, dtype=torch.uint8, device="cuda")
    sp = torch.empty(2 * NS, dtype=torch.int32, device="cuda")
    io = (out.data_ptr(), st.data_ptr(), sp.data_ptr())
    lay = s.layout()
    rec = torch.empty(lay.rows * NS, dtype=torch.int32, device="cuda")
    sync = torch.cuda.synchronize
    sync()

    s.compute_seq(x.reshape(2, NS))
    s.compute(x[:sel.size], index=sel)
    s.compute_ragged(x[:total], cnt, index=sel)
    s.compute_queue(ids, x[:total])
    for call in (
            lambda: s.compute_seq_device(d_x.data_ptr(), 2, *io, stream=sh),
            lambda: s.compute_device(d_x.data_ptr(), *io, stream=sh, index_ptr=d_sel.data_ptr(), m=sel.size),
            lambda: s.compute_ragged_device(d_x.data_ptr(), d_off.data_ptr(), total, *io, stream=sh,
                                            index_ptr=d_sel.data_ptr(), m=sel.size),
            lambda: s.compute_queue_device(d_ids.data_ptr(), d_x.data_ptr(), total, *io, stream=sh)):
        call()
        sync()
    snap = s.snapshot(index=sel)
    s.restore(snap, index=sel)
    s.snapshot_device(rec.data_ptr(), stream=sh)
    sync()
    s.restore_device(lay, rec.data_ptr(), NS, stream=sh)
    sync()
    s.close()


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--fold":
        fold(sys.argv[2])
    else:
        main()
