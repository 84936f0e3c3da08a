// tuning.hpp — tgo_set_tuning's knobs as one table: a value per key and a row per key that says
// which values the key takes.  Host-only and free of HIP, so that a test compiles it alone.  Private.
#pragma once
#include <cstdint>
#include <string>
#include "../../include/titan_gpu_olap.h"

namespace tgo {

constexpr int kTuneKeys = TGO_TUNE_PP_SLOTS + 1;        // the keys are 1 .. kTuneKeys - 1
// engine.hpp's kCoreQueue, kMsHeadMax, kPpMinSlots and kPpMaxSlots (api.cpp asserts that they agree)
constexpr double kTuneCoreQueue = 4096, kTuneMsHeadMax = 1 << 20, kTunePpMinSlots = 16, kTunePpMaxSlots = 1024;
constexpr double kTuneMaxCount = 9.0e15;                // counts stay exact in a double

// What a value below 0 means: an error unless the range holds it / -1 alone is "the default" / every one is.
enum class TuneNeg { none, minus_one, any };
// The value kept: as given / a whole number or an error / the whole part.
enum class TuneNum { real, whole, truncated };

struct TuneRow {
    const char* name;
    double lo, hi;          // the values taken (besides what `neg` adds)
    TuneNum num;
    TuneNeg neg;
    const char* msg;        // tgo_last_error of a value not taken
};

constexpr char kTuneTriRowMsg[] = "TGO_TUNE_TRI_WAVE_ROW / _BLOCK_ROW: a row length >= 1 (< 0: the default)";
constexpr char kTuneSccPhaseMsg[] = "TGO_TUNE_SCC_TRIM / _PIVOT: 0 (the phase is skipped) or 1 (< 0: the default)";
constexpr char kTunePpRowMsg[] = "TGO_TUNE_PP_WAVE_ROW / _BLOCK_ROW: a row length >= 1 (< 0: the default)";

// Row k is key k's.
constexpr TuneRow kTuneRows[kTuneKeys] = {
    {nullptr, 0, 0, TuneNum::real, TuneNeg::none, nullptr},
    {"TGO_TUNE_MS_SPLIT", 0, 1, TuneNum::real, TuneNeg::any, "TGO_TUNE_MS_SPLIT: a fraction <= 1 (< 0: the default)"},
    {"TGO_TUNE_MS_GHOST", 0, 1, TuneNum::whole, TuneNeg::none, "TGO_TUNE_MS_GHOST: 0 or 1"},
    {"TGO_TUNE_DS_BINS", 0, 1, TuneNum::whole, TuneNeg::minus_one, "TGO_TUNE_DS_BINS: 0, 1 or -1"},
    {"TGO_TUNE_DS_PILE_CAP", 0, kTuneMaxCount, TuneNum::truncated, TuneNeg::none, "TGO_TUNE_DS_PILE_CAP: entries >= 0"},
    {"TGO_TUNE_DS_DONE", 0, 1, TuneNum::whole, TuneNeg::minus_one, "TGO_TUNE_DS_DONE: 0, 1 or -1"},
    {"TGO_TUNE_MS_COLD", 0, 2147483646.0, TuneNum::whole, TuneNeg::minus_one,
     "TGO_TUNE_MS_COLD: -1, 0, 1 or a hot-head size > 1"},
    {"TGO_TUNE_DS_PULL", -1, 1, TuneNum::real, TuneNeg::none, "TGO_TUNE_DS_PULL: a fraction in [0, 1] or -1"},
    {"TGO_TUNE_DS_SMALL", 0, 1, TuneNum::whole, TuneNeg::minus_one, "TGO_TUNE_DS_SMALL: 0, 1 or -1"},
    {"TGO_TUNE_MS_STAY", 0, 1.0e18, TuneNum::real, TuneNeg::minus_one,
     "TGO_TUNE_MS_STAY: gamma >= 0 (0 = off) or -1 (the default)"},
    {"TGO_TUNE_MS_SPARSE", 0, 1.0e18, TuneNum::real, TuneNeg::minus_one,
     "TGO_TUNE_MS_SPARSE: a fraction >= 0 (0 = off) or -1 (the default)"},
    {"TGO_TUNE_TRI_WAVE_ROW", 1, kTuneMaxCount, TuneNum::whole, TuneNeg::any, kTuneTriRowMsg},
    {"TGO_TUNE_TRI_BLOCK_ROW", 1, kTuneMaxCount, TuneNum::whole, TuneNeg::any, kTuneTriRowMsg},
    {"TGO_TUNE_MS_HEAD", 0, kTuneMsHeadMax, TuneNum::whole, TuneNeg::minus_one,
     "TGO_TUNE_MS_HEAD: a whole number of entries in [0, 2^20] (0 = off) or -1 (the default)"},
    {"TGO_TUNE_CORE_WAVE_ROW", 1, kTuneMaxCount, TuneNum::whole, TuneNeg::any,
     "TGO_TUNE_CORE_WAVE_ROW: a neighbourhood size >= 1 (< 0: the default)"},
    {"TGO_TUNE_CORE_TAIL", 0, kTuneMaxCount, TuneNum::whole, TuneNeg::any,
     "TGO_TUNE_CORE_TAIL: a whole number of vertices >= 0 (0 = never; < 0: the default)"},
    {"TGO_TUNE_CORE_LDS_QUEUE", 1, kTuneCoreQueue, TuneNum::whole, TuneNeg::any,
     "TGO_TUNE_CORE_LDS_QUEUE: entries in [1, 4096] (< 0: the default)"},
    {"TGO_TUNE_SCC_WAVE_ROW", 1, kTuneMaxCount, TuneNum::whole, TuneNeg::any,
     "TGO_TUNE_SCC_WAVE_ROW: a row length >= 1 (< 0: the default)"},
    {"TGO_TUNE_SCC_TAIL", 0, kTuneMaxCount, TuneNum::whole, TuneNeg::any,
     "TGO_TUNE_SCC_TAIL: a whole number of vertices >= 0 (0 = never; < 0: the default)"},
    {"TGO_TUNE_SCC_TRIM", 0, 1, TuneNum::whole, TuneNeg::any, kTuneSccPhaseMsg},
    {"TGO_TUNE_SCC_PIVOT", 0, 1, TuneNum::whole, TuneNeg::any, kTuneSccPhaseMsg},
    {"TGO_TUNE_BC_WAVE_ROW", 1, kTuneMaxCount, TuneNum::whole, TuneNeg::any,
     "TGO_TUNE_BC_WAVE_ROW: a row length >= 1 (< 0: the default)"},
    {"TGO_TUNE_PP_WAVE_ROW", 1, kTuneMaxCount, TuneNum::whole, TuneNeg::any, kTunePpRowMsg},
    {"TGO_TUNE_PP_BLOCK_ROW", 1, kTuneMaxCount, TuneNum::whole, TuneNeg::any, kTunePpRowMsg},
    {"TGO_TUNE_PP_SLOTS", kTunePpMinSlots, kTunePpMaxSlots, TuneNum::whole, TuneNeg::any,
     "TGO_TUNE_PP_SLOTS: table entries per wave in [16, 1024] (< 0: the default)"},
};

// One value per key (v[key]).  Below 0 = not set: the reader takes the environment variable or the
// default (env.hpp tuned / tuned_on), but for the two keys without a variable, which start at their
// defaults: MS_GHOST on, DS_PILE_CAP 0 (= n entries).  Whole numbers stay below 2^53: exact in a double.
struct Tuning {
    double v[kTuneKeys];
    Tuning() {
        for (double& x : v) x = -1.0;
        v[TGO_TUNE_MS_GHOST] = 1.0;
        v[TGO_TUNE_DS_PILE_CAP] = 0.0;
    }
    double f64(int key) const { return v[key]; }
    int64_t i64(int key) const { return static_cast<int64_t>(v[key]); }
};

// tgo_set_tuning behind its null check: TGO_OK and the value kept, or TGO_E_INVALID and the reason in err.
inline int tuning_set(Tuning& t, int32_t key, double value, std::string& err) {
    if (key < 1 || key >= kTuneKeys) {
        err = "tgo_set_tuning: unknown key";
        return TGO_E_INVALID;
    }
    const TuneRow& row = kTuneRows[key];
    if (value < 0.0 && (row.neg == TuneNeg::any || (row.neg == TuneNeg::minus_one && value == -1.0))) {
        t.v[key] = -1.0;
        return TGO_OK;
    }
    // (NaN fails the first comparison; the cast is made of a value inside the range only)
    if (!(value >= row.lo && value <= row.hi) ||
        (row.num == TuneNum::whole && value != static_cast<double>(static_cast<int64_t>(value)))) {
        err = row.msg;
        return TGO_E_INVALID;
    }
    t.v[key] = row.num == TuneNum::real ? value : static_cast<double>(static_cast<int64_t>(value));
    return TGO_OK;
}

}  // namespace tgo
