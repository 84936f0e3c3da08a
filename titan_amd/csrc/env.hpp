// env.hpp — the one spelling of the environment reads (host code of the .cpp and .hip files).
//
// Every helper reads the environment when it is called.  A caller that wants the value latched
// for the process keeps it in a function-local static (read on the first use of that function);
// a caller whose variable tests flip between calls (TGO_HOST_ASSEMBLY, the TGO_PR_* layout
// variables) calls the helper each time.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdlib>

namespace tgo {

inline int64_t env_i64(const char* name, int64_t dflt) {
    const char* v = std::getenv(name);
    return v ? std::atoll(v) : dflt;
}

inline double env_double(const char* name, double dflt) {
    const char* v = std::getenv(name);
    return v ? std::atof(v) : dflt;
}

// env_double clamped to [lo, hi]; lo when the value is not a number
inline double env_clamped(const char* name, double dflt, double lo, double hi) {
    const double v = env_double(name, dflt);
    return !(v >= lo) ? lo : (v < hi ? v : hi);
}

// TGO_TRACE=1: phase times and per-level lines on stderr (set and a non-zero integer).
inline bool trace_on() { return env_i64("TGO_TRACE", 0) != 0; }

// TGO_HOST_ASSEMBLY=1: CSR assembly and the PageRank layouts on the host, not the device.
inline bool host_assembly() { return env_i64("TGO_HOST_ASSEMBLY", 0) != 0; }

// The tuning rule: a knob's tgo_set_tuning value when one is set (>= 0), else `env` — what the
// environment variable or, without one, the default gives (parsed, clamped and latched by the
// caller: each knob's variable is read once, on the first use of the function that owns it).
inline double tuned(double set, double env) { return set >= 0.0 ? set : env; }
inline int64_t tuned(int64_t set, int64_t env) { return set >= 0 ? set : env; }
// ... for a switch: 0 off, anything else on
inline bool tuned_on(int64_t set, bool env) { return set >= 0 ? set != 0 : env; }

}  // namespace tgo
