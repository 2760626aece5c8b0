// mk_rtc.cpp -- the native tier's run-time compiler: one generated module
// (tis_jit.h) through hiprtc into a gfx950 code object, on compile threads
// with stacks of their own, by the linked hiprtc or by this ROCm's hiprtc in
// link-map namespaces of its own (dlmopen), with a bound after which the
// caller gives up; and the reader of a code object's metadata.  Host only:
// hiprtc.h, libc and pthreads, no HIP runtime call and no kernel, so the unit
// also builds with a plain C++ compiler into the stand-alone driver
// (tests/native/rtc_compile.cpp) that runs it under sanitizers.  mk_rtc.h is
// all the executor sees of it.
//
// Two things here happen outside any call and must stay so:
//   * the teardown drain: g_rtc_drain's destructor, and the
//     atexit(rtc_drain_at_exit) registered when a namespace opens, wait for
//     compiles still running before static destructors (this library's, then
//     the namespaces') run under them.  The drain only covers objects
//     constructed before it: a function-local static first used later (in a
//     compile, say) is destroyed before the drain waits.  Whatever a running
//     compile reads must therefore never be destroyed (as ns_environ_install's
//     map, NsPool::get);
//   * the load-time environment read: g_segv_trace reads MK_SEGV_TRACE once,
//     when the library loads, and installs the signal trace then.
#include "mk_rtc.h"

#include <hip/hiprtc.h>

#include <dlfcn.h>
#include <execinfo.h>
#include <fcntl.h>
#include <pthread.h>
#include <ucontext.h>
#include <sys/syscall.h>
#include <signal.h>
#include <glob.h>
#include <unistd.h>

#include <cerrno>
#include <climits>

extern char **environ;

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <mutex>

namespace mk {
namespace {

// One hiprtc compilation, run on a compile thread so that the caller can
// give up after lim.max_compile_s: the job owns its inputs and outputs
// (shared), so a compile the caller abandoned finishes in the background and
// is discarded.
struct HiprtcJob {
    std::string src;
    std::vector<std::string> env; // the caller's environment, copied on the caller's thread (rtc_compile)
    std::mutex mu;
    std::condition_variable cv;
    bool done = false, ok = false;
    bool abandoned = false; // the caller gave up (under mu)
    std::string why;
    std::vector<char> code;
};

// Compiles still running on detached threads: the library's teardown waits
// for them (a thread inside comgr while static destructors run would crash).
// Diagnostics (MK_SEGV_TRACE=1): a fatal signal in any thread prints that
// thread's native backtrace (library+offset per frame) before the handler
// that was installed before it (Python's faulthandler, say) runs.
struct sigaction g_prev_segv, g_prev_bus, g_prev_abrt;
void segv_trace(int sig, siginfo_t *si, void *uc)
{
    // async-signal-safe after the warm-up at install: no malloc here
    char msg[256];
    const auto *ctx = static_cast<const ucontext_t *>(uc);
    void *pc = ctx ? reinterpret_cast<void *>(ctx->uc_mcontext.gregs[REG_RIP]) : nullptr;
    Dl_info info{};
    const bool named = pc && dladdr(pc, &info) && info.dli_fname;
    char comm[32] = "?";
    {
        char path[64];
        snprintf(path, sizeof path, "/proc/self/task/%ld/comm", (long)syscall(SYS_gettid));
        const int fd = open(path, O_RDONLY);
        if (fd >= 0) {
            const ssize_t r = read(fd, comm, sizeof comm - 1);
            comm[r > 0 ? r - 1 : 0] = 0;
            close(fd);
        }
    }
    const int l = snprintf(msg, sizeof msg, "mk: signal %d at %p in thread %ld (%s), pc %p = %s+%#lx\n", sig,
                           si ? si->si_addr : nullptr, (long)syscall(SYS_gettid), comm, pc,
                           named ? info.dli_fname : "?",
                           named ? (unsigned long)((char *)pc - (char *)info.dli_fbase) : 0ul);
    if (write(2, msg, (size_t)l) < 0) {
    }
    void *frames[64];
    const int n = backtrace(frames, 64);
    backtrace_symbols_fd(frames, n, 2);
    const struct sigaction &prev = sig == SIGSEGV ? g_prev_segv : sig == SIGBUS ? g_prev_bus : g_prev_abrt;
    if ((prev.sa_flags & SA_SIGINFO) && prev.sa_sigaction) {
        prev.sa_sigaction(sig, si, uc);
        return;
    }
    signal(sig, SIG_DFL);
    raise(sig);
}
void segv_trace_install()
{
    struct sigaction sa;
    std::memset(&sa, 0, sizeof sa);
    sa.sa_sigaction = segv_trace;
    sa.sa_flags = SA_SIGINFO | SA_ONSTACK;
    sigaction(SIGSEGV, &sa, &g_prev_segv);
    sigaction(SIGBUS, &sa, &g_prev_bus);
    sigaction(SIGABRT, &sa, &g_prev_abrt);
}
struct SegvTrace {
    SegvTrace()
    {
        const char *e = std::getenv("MK_SEGV_TRACE");
        if (!e || *e != '1') return;
        void *warm[2];
        (void)backtrace(warm, 2); // loads the unwinder now, not inside the handler
        segv_trace_install();
        on = true;
    }
    bool on = false;
} g_segv_trace;

// Diagnostics: a compiler that installed its own fatal-signal handlers is
// named, and ours put back in front of them.
void segv_trace_check()
{
    if (!g_segv_trace.on) return;
    struct sigaction cur;
    if (sigaction(SIGSEGV, nullptr, &cur) || cur.sa_sigaction == segv_trace) return;
    Dl_info info{};
    const bool named = dladdr(reinterpret_cast<void *>(cur.sa_sigaction), &info) && info.dli_fname;
    fprintf(stderr, "mk: SIGSEGV handler replaced by %s; reinstalled\n", named ? info.dli_fname : "?");
    segv_trace_install();
}

// Compile threads: detached, with a stack of their own size.  Clang and LLVM
// recurse deeply on long generated sources; a thread's default stack is the
// stack rlimit (8 MiB here) or 2 MiB where that rlimit is unlimited, less
// than the main thread of a compiler process gets.  With MK_SEGV_TRACE the
// thread also gets an alternate signal stack, so an overflow is reported.
constexpr size_t kCompileStack = (size_t)256 << 20;

void *compile_thread_main(void *arg)
{
    std::unique_ptr<std::function<void()>> f(static_cast<std::function<void()> *>(arg));
    if (g_segv_trace.on) {
        stack_t ss{};
        ss.ss_size = 1 << 16;
        ss.ss_sp = std::malloc(ss.ss_size); // held for the thread's life
        if (ss.ss_sp) (void)sigaltstack(&ss, nullptr);
    }
    (*f)();
    return nullptr;
}

bool spawn_compile_thread(std::function<void()> fn)
{
    auto *f = new std::function<void()>(std::move(fn));
    pthread_attr_t a;
    pthread_attr_init(&a);
    pthread_attr_setstacksize(&a, kCompileStack);
    pthread_attr_setdetachstate(&a, PTHREAD_CREATE_DETACHED);
    pthread_t t;
    const int rc = pthread_create(&t, &a, compile_thread_main, f);
    pthread_attr_destroy(&a);
    if (rc) {
        // no thread: run here (the caller's stack)
        std::unique_ptr<std::function<void()>> own(f);
        (*own)();
        return false;
    }
    return true;
}

std::mutex g_rtc_mu;
std::condition_variable g_rtc_cv;
int g_rtc_running = 0;
void rtc_drain_at_exit()
{
    std::unique_lock<std::mutex> lk(g_rtc_mu);
    (void)g_rtc_cv.wait_for(lk, std::chrono::seconds(120), [] { return g_rtc_running == 0; });
}
struct RtcDrain {
    ~RtcDrain() { rtc_drain_at_exit(); }
} g_rtc_drain;

// The native tier's compiler is this ROCm install's hiprtc, always: a cgo or
// C caller links it, and so does this library.  But in a process that
// imported PyTorch first, PyTorch's bundled libhiprtc / libamd_comgr (the
// same sonames, an older LLVM) are what the linked hiprtc symbols resolve to
// -- a different compiler, whose code differs from network to network (C4
// D=256: 132 VGPRs against 75).  There this ROCm's libhiprtc is opened a
// second time in a link-map namespace of its own (dlmopen LM_ID_NEWLM: its
// libamd_comgr, libstdc++ and libc come with it, invisible to the rest of
// the process), and the module is compiled in process by that copy, so
// every caller gets the same module without a child process.
//
// Round 3 compiled such modules in a child process (posix_spawn from a
// compile thread of a GPU-initialised process); the host heap of those
// PyTorch processes was found corrupted at exit.  Round 5
// removed that path: this library starts no process.  MK_HIPRTC=linked
// compiles with whatever hiprtc the process resolved (PyTorch's in a PyTorch
// process), MK_HIPRTC=ns with the namespace copy; any other value is refused
// (the network stays on tier 2, the plan says why).
#ifndef MK_ROCM_LIB
#define MK_ROCM_LIB "/opt/rocm/lib"
#endif

enum RtcKind { RTC_LINKED, RTC_NS, RTC_REFUSED };

struct RtcChoice {
    RtcKind kind = RTC_LINKED;
    std::string why; // RTC_REFUSED: the reason
};

// Whether the linked hiprtc is another install's than this ROCm's (PyTorch's
// bundled one in a process that imported it first).
bool inproc_rtc_differs()
{
    Dl_info info{};
    if (!dladdr(reinterpret_cast<void *>(&hiprtcCompileProgram), &info) || !info.dli_fname) return false;
    char real[PATH_MAX], want[PATH_MAX];
    if (!realpath(info.dli_fname, real) || !realpath(MK_ROCM_LIB, want)) return true;
    const size_t n = std::strlen(want);
    return std::strncmp(real, want, n) != 0 || real[n] != '/';
}

RtcChoice rtc_choice()
{
    RtcChoice c;
    const char *e = std::getenv("MK_HIPRTC");
    if (e && *e) {
        if (!std::strcmp(e, "linked")) return c;
        if (!std::strcmp(e, "ns")) {
            c.kind = RTC_NS;
            return c;
        }
        c.kind = RTC_REFUSED; // the round-3 helper process (=helper / =<path>) was removed
        c.why = std::string("MK_HIPRTC=") + e + " refused: only linked and ns compile (no helper process)";
        return c;
    }
    if (inproc_rtc_differs()) c.kind = RTC_NS;
    return c;
}

// The hiprtc entry points one compile uses: the linked ones, or this ROCm's
// in its own namespace.
struct RtcApi {
    decltype(&hiprtcCreateProgram) create;
    decltype(&hiprtcCompileProgram) compile;
    decltype(&hiprtcGetProgramLogSize) log_size;
    decltype(&hiprtcGetProgramLog) log;
    decltype(&hiprtcGetCodeSize) code_size;
    decltype(&hiprtcGetCode) code;
    decltype(&hiprtcDestroyProgram) destroy;
    decltype(&hiprtcGetErrorString) error;
    char ***environ_ns = nullptr; // the namespace libc's environ (null: the linked one)
};

const RtcApi kLinkedRtc = {&hiprtcCreateProgram, &hiprtcCompileProgram, &hiprtcGetProgramLogSize,
                           &hiprtcGetProgramLog, &hiprtcGetCodeSize,    &hiprtcGetCode,
                           &hiprtcDestroyProgram, &hiprtcGetErrorString};

// Namespaces the compiler may open: one per compile worker (NsPool).
constexpr size_t kNsMax = 4;

// This ROCm's libhiprtc: the versioned sonames under MK_ROCM_LIB, highest
// first (libhiprtc.so.7 on ROCm 7.x), then the unversioned link.
std::vector<std::string> hiprtc_candidates()
{
    std::vector<std::string> v;
    glob_t g{};
    if (glob(MK_ROCM_LIB "/libhiprtc.so.[0-9]*", 0, nullptr, &g) == 0)
        for (size_t i = 0; i < g.gl_pathc; i++) v.emplace_back(g.gl_pathv[i]);
    globfree(&g);
    // libhiprtc.so.7 before libhiprtc.so.7.2.x: the soname before the file
    std::sort(v.begin(), v.end(), [](const std::string &a, const std::string &b) {
        return a.size() != b.size() ? a.size() < b.size() : a > b;
    });
    v.emplace_back(MK_ROCM_LIB "/libhiprtc.so");
    return v;
}

// This ROCm's hiprtc in namespace k, opened on first use (by worker k's
// thread, see NsCompiler) and never closed; null (with the reason) when it
// cannot be opened.
const RtcApi *ns_rtc(size_t k, std::string &why)
{
    static std::string fail[kNsMax];
    static const RtcApi *api[kNsMax];
    static std::once_flag once[kNsMax];
    std::call_once(once[k], [k] { api[k] = [k]() -> const RtcApi * {
        void *h = nullptr;
        std::string errs;
        for (const std::string &path : hiprtc_candidates()) {
            if ((h = dlmopen(LM_ID_NEWLM, path.c_str(), RTLD_NOW | RTLD_LOCAL))) break;
            const char *d = dlerror();
            errs += (errs.empty() ? "" : "; ") + std::string(d ? d : path + ": failed");
        }
        if (!h) {
            fail[k] = "dlmopen: " + errs;
            return nullptr;
        }
        auto *a = new RtcApi{};
        a->create = reinterpret_cast<decltype(a->create)>(dlsym(h, "hiprtcCreateProgram"));
        a->compile = reinterpret_cast<decltype(a->compile)>(dlsym(h, "hiprtcCompileProgram"));
        a->log_size = reinterpret_cast<decltype(a->log_size)>(dlsym(h, "hiprtcGetProgramLogSize"));
        a->log = reinterpret_cast<decltype(a->log)>(dlsym(h, "hiprtcGetProgramLog"));
        a->code_size = reinterpret_cast<decltype(a->code_size)>(dlsym(h, "hiprtcGetCodeSize"));
        a->code = reinterpret_cast<decltype(a->code)>(dlsym(h, "hiprtcGetCode"));
        a->destroy = reinterpret_cast<decltype(a->destroy)>(dlsym(h, "hiprtcDestroyProgram"));
        a->error = reinterpret_cast<decltype(a->error)>(dlsym(h, "hiprtcGetErrorString"));
        a->environ_ns = reinterpret_cast<char ***>(dlsym(h, "__environ"));
        if (!a->create || !a->compile || !a->log_size || !a->log || !a->code_size || !a->code || !a->destroy ||
            !a->error || !a->environ_ns) {
            fail[k] = "dlmopen: hiprtc symbols missing";
            delete a;
            return nullptr;
        }
        // The namespace's static destructors were registered with exit()
        // while it loaded; a compile still running must end before they run,
        // so this drain (registered after them) runs first.
        (void)std::atexit(rtc_drain_at_exit);
        return a;
    }(); });
    why = fail[k];
    return api[k];
}

// Every compile in a namespace runs on one thread, which also opens it, and
// which never exits.  The namespace's libc keeps per-thread state (ctype
// tables, malloc's thread cache, thread_local destructor lists) that only
// the opening thread gets initialised, and that threads started by the
// process's own libc leave behind unrun when they end: compiles on
// short-lived threads crashed now and then in comgr (r04a, CPU reproduction).
class NsCompiler {
  public:
    explicit NsCompiler(size_t k) : k_(k) { spawn_compile_thread([this] { loop(); }); }
    size_t index() const { return k_; }
    // Queues f for the compile thread and returns when it has run.
    void run(const std::shared_ptr<HiprtcJob> &j, const std::function<void()> &f)
    {
        auto done = std::make_shared<std::pair<std::mutex, std::condition_variable>>();
        bool finished = false;
        {
            std::lock_guard<std::mutex> lk(mu_);
            q_.push_back({j, [&f, &finished, done] {
                              f();
                              std::lock_guard<std::mutex> g(done->first);
                              finished = true;
                              done->second.notify_all();
                          }});
        }
        cv_.notify_one();
        std::unique_lock<std::mutex> lk(done->first);
        done->second.wait(lk, [&] { return finished; });
    }
    // Busy with a compile its caller has given up on (rtc_compile's bound):
    // a job queued here would wait for it.
    bool stuck()
    {
        std::shared_ptr<HiprtcJob> cur;
        {
            std::lock_guard<std::mutex> lk(mu_);
            cur = cur_;
        }
        if (!cur) return false;
        std::lock_guard<std::mutex> g(cur->mu);
        return cur->abandoned;
    }

  private:
    void loop()
    {
        for (;;) {
            std::pair<std::shared_ptr<HiprtcJob>, std::function<void()>> job;
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [this] { return !q_.empty(); });
                job = std::move(q_.front());
                q_.pop_front();
                cur_ = job.first;
            }
            job.second();
            {
                std::lock_guard<std::mutex> lk(mu_);
                cur_.reset();
            }
            segv_trace_check();
        }
    }
    size_t k_;
    std::mutex mu_;
    std::condition_variable cv_;
    std::deque<std::pair<std::shared_ptr<HiprtcJob>, std::function<void()>>> q_;
    std::shared_ptr<HiprtcJob> cur_; // the job running now (under mu_)
};

// The namespace compile workers.  A compile that outlives its bound keeps
// its worker (and that copy of LLVM) busy until it ends; the next compile
// goes to the first worker that is not stuck so, opening another namespace
// (up to kNsMax) when all are -- before, one pathological module held up
// every later network's compile until its own bound, each then falling
// back to tier 2 (r05c: a 282-variant census network).  Workers never exit.
class NsPool {
  public:
    static NsPool &get()
    {
        static NsPool *p = new NsPool(); // never destroyed: the threads outlive every caller
        return *p;
    }
    NsCompiler &pick()
    {
        std::lock_guard<std::mutex> lk(mu_);
        for (NsCompiler *w : ws_)
            if (!w->stuck()) return *w;
        if (ws_.size() < kNsMax) {
            ws_.push_back(new NsCompiler(ws_.size()));
            return *ws_.back();
        }
        return *ws_.front(); // all stuck: wait behind the first
    }

  private:
    std::mutex mu_;
    std::vector<NsCompiler *> ws_;
};

// A linked (in-process, this namespace) compile that outlived its bound:
// the next compile takes a namespace worker instead of queueing behind it
// in the same comgr.
std::mutex g_linked_mu;
std::vector<std::weak_ptr<HiprtcJob>> g_linked_running;

bool linked_stuck()
{
    std::lock_guard<std::mutex> lk(g_linked_mu);
    for (auto &w : g_linked_running)
        if (auto j = w.lock()) {
            std::lock_guard<std::mutex> g(j->mu);
            if (j->abandoned && !j->done) return true;
        }
    return false;
}

bool write_file(const std::string &path, const std::string &data)
{
    const int fd = open(path.c_str(), O_WRONLY | O_CREAT | O_EXCL | O_CLOEXEC, 0600);
    if (fd < 0) return false;
    size_t off = 0;
    while (off < data.size()) {
        const ssize_t w = write(fd, data.data() + off, data.size() - off);
        if (w < 0 && errno == EINTR) continue;
        if (w <= 0) break;
        off += (size_t)w;
    }
    return close(fd) == 0 && off == data.size();
}

// Code object version of the native tier's modules: v5, which every HIP runtime a caller may bring understands.  ROCm
// 7.2's hiprtc defaults to v6; loaded into PyTorch's bundled (ROCm 7.0) HIP
// runtime, v6 modules of the machine shape left the host heap corrupted at
// process exit (free(): corrupted unsorted chunks after 60 dynamic-stack
// networks, r03c-r03k), v5 ones and the bundled compiler's did not.
constexpr const char *kCodeObjectVersion = "-mcode-object-version=5";

// The namespace's libc took the process's environment pointer when it was
// opened, and setenv (os.environ[...] = ... in Python) later reallocates and
// frees that array: comgr's getenv then read freed memory (r04: SIGSEGV in
// the compile thread after a test's monkeypatch.setenv).  Each compile gives
// the namespace a private copy of the environment instead: copied from
// `environ` on the caller's thread when the compile is requested
// (rtc_compile, so no compile thread walks the process's array while another
// thread may setenv), installed by the compile thread, which alone reads it.
std::vector<std::string> environ_snapshot()
{
    std::vector<std::string> s;
    for (char **e = environ; e && *e; ++e) s.emplace_back(*e);
    return s;
}

void ns_environ_install(const RtcApi &rt, const std::vector<std::string> &snapshot)
{
    // one copy per namespace (its worker alone refreshes it): a refresh for
    // one namespace must not free the strings another's compile still reads
    struct Env {
        std::vector<std::string> strings;
        std::vector<char *> ptrs;
    };
    static std::mutex mu;
    // never destroyed: registered with exit() after the teardown drain, the
    // map would go before the drain waits, under a compile that still reads
    // its strings (SIGSEGV in comgr's getenv at exit, stand-alone driver)
    static auto *envs = new std::map<char ***, Env>();
    Env *env;
    {
        std::lock_guard<std::mutex> lk(mu);
        env = &(*envs)[rt.environ_ns]; // map nodes are stable
    }
    std::vector<std::string> &strings = env->strings;
    std::vector<char *> &ptrs = env->ptrs;
    std::vector<std::string> s(snapshot);
    std::vector<char *> p;
    p.reserve(s.size() + 1);
    for (std::string &x : s) p.push_back(&x[0]);
    p.push_back(nullptr);
    *rt.environ_ns = p.data(); // the new copy is complete before the old one goes
    strings.swap(s);
    ptrs.swap(p);
}

// In-process hiprtc (the linked symbols, or this ROCm's namespace copy).
void rtc_inproc(const RtcApi &rt, const HiprtcJob &j, bool &ok, std::string &why, std::vector<char> &code)
{
    if (rt.environ_ns) ns_environ_install(rt, j.env);
    const std::string &src = j.src;
    hiprtcProgram prog;
    if (rt.create(&prog, src.c_str(), "mk_jit.hip", 0, nullptr, nullptr) != HIPRTC_SUCCESS) {
        why = "hiprtcCreateProgram failed";
        return;
    }
    const char *opts[] = {"--offload-arch=gfx950", "-O3", "-std=c++17", kCodeObjectVersion};
    const hiprtcResult r = rt.compile(prog, 4, opts);
    size_t cs = 0;
    if (r != HIPRTC_SUCCESS) {
        size_t ls = 0;
        (void)rt.log_size(prog, &ls);
        std::string log(ls, '\0');
        if (ls) (void)rt.log(prog, &log[0]);
        why = std::string("hiprtc: ") + rt.error(r) + ": " + log.substr(0, 400);
    } else if (rt.code_size(prog, &cs) != HIPRTC_SUCCESS || cs == 0) {
        why = "hiprtc produced no code";
    } else {
        code.resize(cs);
        (void)rt.code(prog, code.data());
        ok = true;
    }
    (void)rt.destroy(&prog);
}

bool rtc_abandoned(HiprtcJob &j)
{
    std::lock_guard<std::mutex> lk(j.mu);
    return j.abandoned;
}

// The namespace compiler could not be opened (its reason, e.g. the dlmopen
// error): modules then come from the linked hiprtc ("linked-other" in a
// PyTorch process, whose code differs).  Said once on stderr
// and kept for mk_net_plan (rtc_ns_error=).
std::mutex g_ns_fail_mu;
std::string g_ns_fail;

void ns_degraded(const std::string &why)
{
    std::lock_guard<std::mutex> lk(g_ns_fail_mu);
    if (!g_ns_fail.empty()) return;
    g_ns_fail = why.empty() ? std::string("namespace compiler unavailable") : why;
    fprintf(stderr, "mk: native-tier namespace compiler unavailable (%s); compiling with the linked hiprtc\n",
            g_ns_fail.c_str());
}
} // namespace

std::string ns_fail_reason()
{
    std::lock_guard<std::mutex> lk(g_ns_fail_mu);
    return g_ns_fail;
}

namespace {

// One compile with the chosen compiler.  The linked hiprtc is the fallback
// when the chosen one cannot run -- unless the caller has given up by then,
// whose result nobody would read.
void hiprtc_run(const std::shared_ptr<HiprtcJob> &j)
{
    bool ok = false;
    std::string why;
    std::vector<char> code;
    const RtcChoice ch = rtc_choice();
    bool ran = false;
    std::string from;
    if (ch.kind == RTC_REFUSED) {
        ran = true; // nothing compiles: the network stays on tier 2
        why = ch.why;
    } else if (ch.kind == RTC_NS || (ch.kind == RTC_LINKED && linked_stuck())) {
        NsCompiler &w = NsPool::get().pick();
        w.run(j, [&] {
            if (const RtcApi *rt = ns_rtc(w.index(), why)) {
                rtc_inproc(*rt, *j, ok, why, code);
                ran = true;
                from = "ns";
            }
        });
        if (!ran) ns_degraded(why);
    }
    if (!ran && !rtc_abandoned(*j)) {
        why.clear();
        {
            std::lock_guard<std::mutex> lk(g_linked_mu);
            g_linked_running.erase(std::remove_if(g_linked_running.begin(), g_linked_running.end(),
                                                  [](const std::weak_ptr<HiprtcJob> &w) { return w.expired(); }),
                                   g_linked_running.end());
            g_linked_running.push_back(j);
        }
        rtc_inproc(kLinkedRtc, *j, ok, why, code);
        from = inproc_rtc_differs() ? "linked-other" : "linked";
    }
    if (ok) why = from; // which compiler's module (mk_net_plan)
    {
        std::lock_guard<std::mutex> lk(j->mu);
        j->ok = ok;
        j->why = std::move(why);
        j->code = std::move(code);
        j->done = true;
        j->cv.notify_all();
    }
    std::lock_guard<std::mutex> lk(g_rtc_mu);
    --g_rtc_running;
    g_rtc_cv.notify_all();
}
} // namespace

uint64_t src_hash(const std::string &src)
{
    uint64_t h = 0xcbf29ce484222325ull; // FNV-1a
    for (unsigned char ch : src) h = (h ^ ch) * 0x100000001b3ull;
    return h;
}

// One module through hiprtc_run on a compile thread, abandoned after max_s
// seconds (`why` says so).  `from` = which compiler built it.
bool rtc_compile(const std::string &src, double max_s, std::vector<char> &code, std::string &why, std::string &from)
{
    auto job = std::make_shared<HiprtcJob>();
    job->src = src;
    job->env = environ_snapshot(); // on the caller's thread (ns_environ_install)
    if (const char *d = std::getenv("MK_JIT_DUMP_SRC"); d && *d) { // diagnostics: every source, before it compiles
        char name[64];
        snprintf(name, sizeof name, "/%016llx.hip", (unsigned long long)src_hash(src));
        (void)write_file(std::string(d) + name, src);
    }
    {
        std::lock_guard<std::mutex> lk(g_rtc_mu);
        ++g_rtc_running;
    }
    spawn_compile_thread([job] { hiprtc_run(job); });
    std::unique_lock<std::mutex> lk(job->mu);
    const auto limit = std::chrono::duration<double>(max_s);
    if (!job->cv.wait_for(lk, limit, [&] { return job->done; })) {
        job->abandoned = true; // the compile runs out in the background, its result discarded
        char b[128];
        snprintf(b, sizeof b, "hiprtc did not finish within the native tier's compile bound (%.0f s)", max_s);
        why = b;
        return false;
    }
    if (!job->ok) {
        why = job->why;
        return false;
    }
    code = std::move(job->code);
    from = job->why; // the compiler whose module this is (hiprtc_run)
    return true;
}

// A numeric field of a code object's AMDGPU metadata (the msgpack note:
// ".vgpr_count", ".agpr_count", ".private_segment_fixed_size"; the native
// modules hold one kernel), or -1.
int64_t co_meta(const std::vector<char> &co, const char *key)
{
    const size_t n = std::strlen(key);
    if (!n || n > 31) return -1;
    const std::string pat = std::string(1, (char)(0xa0u | (unsigned)n)) + key, img(co.begin(), co.end());
    const size_t at = img.find(pat);
    if (at == std::string::npos || at + pat.size() >= img.size()) return -1;
    const size_t i = at + pat.size();
    const uint8_t b = (uint8_t)img[i];
    auto be = [&](size_t k) -> int64_t {
        if (i + k >= img.size()) return -1;
        uint64_t v = 0;
        for (size_t j = 1; j <= k; ++j) v = v << 8 | (uint8_t)img[i + j];
        return (int64_t)v;
    };
    if (b < 0x80u) return b;
    if (b == 0xccu) return be(1);
    if (b == 0xcdu) return be(2);
    if (b == 0xceu) return be(4);
    return -1;
}

// Whether a module holds `waves` waves per SIMD: VGPRs + AGPRs in 8-register
// granules within gfx950's 512 per SIMD lane (`vgpr_file`:
// JitLimits::vgpr_file, lowered only by the tests that take the fallback
// path), and no scratch.  `note` says what was found.
bool module_holds(const std::vector<char> &co, uint32_t waves, uint32_t vgpr_file, std::string &note)
{
    const int64_t v = co_meta(co, ".vgpr_count"), a = co_meta(co, ".agpr_count"),
                  ps = co_meta(co, ".private_segment_fixed_size");
    const int64_t alloc = (v + 7) / 8 * 8 + (std::max<int64_t>(a, 0) + 7) / 8 * 8;
    char b[96];
    snprintf(b, sizeof b, "w%u:v%lld,a%lld,s%lld", waves, (long long)v, (long long)a, (long long)ps);
    note = b;
    return v >= 0 && ps == 0 && alloc * (int64_t)waves <= (int64_t)vgpr_file;
}

} // namespace mk
