// mk_rtc.h -- the native tier's run-time compiler (mk_rtc.cpp): what the
// executor (mk_exec.hip) uses of it.  Host only.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

namespace mk {

// One module through hiprtc on a compile thread, abandoned after max_s
// seconds (`why` says so).  `from` = which compiler built it: "linked",
// "linked-other" or "ns".
bool rtc_compile(const std::string &src, double max_s, std::vector<char> &code, std::string &why, std::string &from);

// FNV-1a of a module source: names its dump (MK_JIT_DUMP_SRC) and its profile.
uint64_t src_hash(const std::string &src);

// A numeric field of a code object's AMDGPU metadata (".vgpr_count", ...), or -1.
int64_t co_meta(const std::vector<char> &co, const char *key);

// Whether a module holds `waves` waves per SIMD within `vgpr_file` registers
// per lane, without scratch.  `note` says what was found.
bool module_holds(const std::vector<char> &co, uint32_t waves, uint32_t vgpr_file, std::string &note);

// Why the namespace compiler could not be opened, or empty (mk_net_plan).
std::string ns_fail_reason();

} // namespace mk
