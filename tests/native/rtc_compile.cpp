// rtc_compile.cpp -- TEST TOOL (not part of the product): a stand-alone
// driver over the product's run-time compiler (csrc/mk_rtc.cpp, linked in
// whole), in a process of its own that never loads PyTorch or the HIP runtime.
// It holds no hiprtc call of its own: every compile is mk::rtc_compile's.
//
//   rtc_compile SOURCE_FILE CODE_OBJECT_FILE
//       compiles one generated module (tis_jit.h jit_module_source / the
//       session module) for gfx950 as the executor would (MK_HIPRTC is
//       honoured) and writes the code object.  Exit status 0 = code written,
//       the compiler that built it ("linked", "ns") on stdout; otherwise the
//       reason is on stdout.
//   rtc_compile meta CODE_OBJECT_FILE KEY...
//       prints "KEY VALUE" per key: mk::co_meta of the code object.
//   rtc_compile stress
//       a fixed scenario of concurrent, bounded and abandoned compiles in one
//       process (below); prints one RESULT line, exit status 0 only if every
//       step held.
//
// Tests use it (built by tests/schedcheck.py rtc_tool, plain or with
// AddressSanitizer + UndefinedBehaviorSanitizer) to check that the generated
// sources compile without a GPU, that the namespace compiler (mk_rtc.cpp
// ns_rtc) inside a PyTorch process yields byte-identical code objects, and to
// run the compile threads, the namespaces, the environment copy and the
// teardown drain under sanitizers, which cannot see code loaded into Python.
// Until round 5 the product ran this tool's predecessor as a child process of
// a GPU-initialised process (MK_HIPRTC=helper); that path was removed
// (DESIGN.md 4b).
#include "../../misaka-net_amd/csrc/mk_rtc.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

namespace {

bool read_file(const char *path, std::string &data)
{
    std::ifstream in(path, std::ios::binary);
    std::stringstream ss;
    ss << in.rdbuf();
    data = ss.str();
    return (bool)in;
}

int compile_file(const char *src_path, const char *out_path)
{
    std::string src;
    if (!read_file(src_path, src) || src.empty()) {
        std::printf("rtc_compile: empty source %s\n", src_path);
        return 2;
    }
    std::vector<char> code;
    std::string why, from;
    // the caller's own time limit decides: an hour is none
    if (!mk::rtc_compile(src, 3600.0, code, why, from)) {
        std::printf("%s\n", why.c_str());
        return 1;
    }
    std::ofstream out(out_path, std::ios::binary);
    out.write(code.data(), (std::streamsize)code.size());
    out.close();
    if (!out) {
        std::printf("rtc_compile: cannot write %s\n", out_path);
        return 1;
    }
    std::printf("%s\n", from.c_str());
    return 0;
}

int meta(const char *co_path, int nkeys, char **keys)
{
    std::string img;
    if (!read_file(co_path, img) || img.empty()) {
        std::printf("rtc_compile: empty code object %s\n", co_path);
        return 2;
    }
    const std::vector<char> co(img.begin(), img.end());
    for (int i = 0; i < nkeys; ++i) std::printf("%s %lld\n", keys[i], (long long)mk::co_meta(co, keys[i]));
    return 0;
}

// Small built-in kernels, distinct by a constant: no two equal sources, so
// no compile is served from another's result.
std::string kernel(int c)
{
    return "extern \"C\" __global__ void mk_stress(int *o, int n)\n{\n"
           "    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);\n"
           "    if (i < n) o[i] = o[i] * 3 + " + std::to_string(1000 + c) + ";\n}\n";
}

struct Outcome {
    bool ok = false;
    std::string why, from;
};

Outcome compile(int c, double max_s)
{
    Outcome o;
    std::vector<char> code;
    o.ok = mk::rtc_compile(kernel(c), max_s, code, o.why, o.from) && !code.empty();
    return o;
}

constexpr double kBound = 600.0;

int stress()
{
    int c = 0;
    std::string failed;
    auto fail = [&](const char *step, const Outcome &o) {
        if (!failed.empty()) return;
        failed = std::string(step) + ": ok=" + (o.ok ? "1" : "0") + " from=" + o.from + " why=" + o.why;
    };
    // 1. four threads, three compiles each: all succeed, one compiler
    constexpr int kThreads = 4, kEach = 3;
    std::vector<Outcome> got(kThreads * kEach);
    {
        std::vector<std::thread> ts;
        for (int t = 0; t < kThreads; ++t)
            ts.emplace_back([&got, t] {
                for (int k = 0; k < kEach; ++k) got[t * kEach + k] = compile(t * kEach + k, kBound);
            });
        for (std::thread &t : ts) t.join();
        c = kThreads * kEach;
    }
    const std::string from = got[0].from;
    for (const Outcome &o : got)
        if (!o.ok || o.from.empty() || o.from != from) fail("concurrent", o);
    // 2. setenv reallocates the environment array between two compiles
    const Outcome before = compile(c++, kBound);
    for (int i = 0; i < 200; ++i) {
        const std::string name = "MK_STRESS_" + std::to_string(i);
        if (setenv(name.c_str(), std::string(50, 'y').c_str(), 1)) failed = "setenv failed";
    }
    const Outcome after = compile(c++, kBound);
    if (!before.ok) fail("before-setenv", before);
    if (!after.ok) fail("after-setenv", after);
    // 3. a compile past its bound is given up, and the next one does not
    // wait behind it: a namespace worker takes it.  A namespace compile
    // runs whether or not its caller has gone, and the next one is "ns" in
    // any case.  A linked compile whose caller gave up before the compile thread
    // looked (hiprtc_run, rtc_abandoned) is never started: whether the 0 s
    // bound or the thread gets there first is a race, nothing is stuck when
    // the bound does, and the next compile is then rightly "linked".
    const Outcome given_up = compile(c++, 0.0);
    if (given_up.ok || given_up.why.find("compile bound") == std::string::npos) fail("bound", given_up);
    const Outcome next = compile(c++, kBound);
    if (!next.ok || (next.from != "ns" && (from != "linked" || next.from != "linked"))) fail("after-bound", next);
    std::printf("RESULT %s from=%s next=%s%s%s\n", failed.empty() ? "ok" : "FAILED", from.c_str(), next.from.c_str(),
                failed.empty() ? "" : " ", failed.c_str());
    std::fflush(stdout);
    // 4. return at once: an abandoned namespace compile may still run, and
    // the teardown drain waits for it.  An abandoned linked compile, if it
    // started at all, has ended by now (the next one opened a namespace
    // meanwhile): exit under a running linked compile is not shown here.
    return failed.empty() ? 0 : 1;
}

} // namespace

int main(int argc, char **argv)
{
    if (argc == 2 && !std::strcmp(argv[1], "stress")) return stress();
    if (argc >= 4 && !std::strcmp(argv[1], "meta")) return meta(argv[2], argc - 3, argv + 3);
    if (argc == 3) return compile_file(argv[1], argv[2]);
    std::printf("usage: rtc_compile SOURCE_FILE CODE_OBJECT_FILE\n"
                "       rtc_compile meta CODE_OBJECT_FILE KEY...\n"
                "       rtc_compile stress\n");
    return 2;
}
