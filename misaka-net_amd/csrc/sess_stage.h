// sess_stage.h -- how a session set cuts its allocations into arrays: the
// carver every one of them goes through (the interpreter's state, the native
// tier's, the queue scratch) and the layout of the host forms' staging.  Host
// arithmetic only, no HIP: mk_exec.hip uses it on the device buffers and
// sched_check.cpp exports it to the CPU tests, where a bad offset is caught
// before it can become an access out of bounds on the GPU.
#pragma once

#include <cstddef>
#include <cstdint>

namespace mk {

// A bump allocator over one allocation, every array at a multiple of 256
// bytes.  Two passes: over a null base `at` ends as the bytes to allocate (the
// pointers mean nothing), over the allocation take() hands out the arrays.
struct Carver {
    char *base;
    size_t at = 0;
    explicit Carver(void *b = nullptr) : base((char *)b) {}
    static size_t al(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
    // the offset of the next `bytes` bytes
    size_t skip(size_t bytes)
    {
        const size_t o = at;
        at += al(bytes);
        return o;
    }
    template <class T>
    T *take(size_t count)
    {
        const size_t o = skip(count * sizeof(T));
        return base ? (T *)(base + o) : nullptr;
    }
};

// The staging of a host form (d_stage and its pinned mirror, the same offsets
// in both): the I/O arrays of c words each, then the extras a form asks for.
// An extra that is absent takes no room; its offset is not to be used.
struct StageLayout {
    size_t in, out, steps, status; // int64, int32, uint32, uint8: c of each
    size_t off;                    // uint32[m + 1], a ragged burst's offsets
    size_t sel;                    // uint32[m], the index list
    size_t ids;                    // uint32[c], a queue's instance numbers
    size_t flag;                   // uint32, the queue's busy flag
    size_t bytes;
};

inline StageLayout stage_layout(size_t c, size_t m, bool sel, bool off, bool ids, bool flag)
{
    Carver k;
    StageLayout L{};
    L.in = k.skip(c * 8);
    L.out = k.skip(c * 4);
    L.steps = k.skip(c * 4);
    L.status = k.skip(c);
    L.off = k.skip(off ? (m + 1) * 4 : 0);
    L.sel = k.skip(sel ? m * 4 : 0);
    L.ids = k.skip(ids ? c * 4 : 0);
    L.flag = k.skip(flag ? 4 : 0);
    L.bytes = k.at;
    return L;
}

} // namespace mk
