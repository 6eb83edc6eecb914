// ba_wave3.hip -- WAVE engine, effective depth 3 (k_om3w), and the engine
// dispatch.
#include "ba_wave.hpp"

// lab A/B builds only (tools/lab_variant.sh -DBA_OM3W_LAB_DIAG=...): k_om3w's DIAG switches
#ifndef BA_OM3W_LAB_DIAG
#define BA_OM3W_LAB_DIAG 0
#endif

namespace ba {

hipError_t launch_wave4(const RunArgs& a, const Geometry& g);  // ba_wave4.hip

// Trees the WAVE kernels are compiled for (k_om3w / k_om4w instantiations).
bool wave_supported(const Geometry& g) {
    return (g.me == 3 && g.n >= 5 && g.n <= 14) || (g.me == 4 && g.n >= 6 && g.n <= kWave4MaxN);
}

hipError_t launch_wave3t(const RunArgs& a);                   // ba_wave3t.hip (n = 10)

// k_om3wt's pair table holds ONE upper half of the global trial-word index: the
// launch may use it when every word its tasks touch (the last task padded to a
// whole one) shares that half.  BA_OM3W_TABLE=0 (read per call: tests and A/B
// runs switch it in-process) keeps k_om3w.
template <int W>
static bool pair_table_applies(const RunArgs& a) {
    if (const char* e = getenv("BA_OM3W_TABLE"))
        if (atoi(e) == 0) return false;
    const uint64_t words = (a.batch + 63) / 64, tasks = (words + W - 1) / W;
    if (tasks == 0) return false;
    const uint64_t first = a.first_trial >> 6, last = first + tasks * W - 1;
    return last >= first && (first >> 32) == (last >> 32);
}

hipError_t launch_wave_engine(const RunArgs& a, const Geometry& g) {
    if (g.me == 4) return launch_wave4(a, g);
    if (g.me != 3) return hipErrorInvalidValue;
    if (g.n == 10 && pair_table_applies<Om3W<10>::W>(a)) return launch_wave3t(a);
    // depth 3: k_om3w (the rejected alternatives live in tools/lab_kernels.hpp)
    switch (g.n) {
#define OM3W_CASE(nn) \
    case nn: return launch_wave<Om3W<nn>>(a, k_om3w<nn, BA_OM3W_LAB_DIAG>, "k_om3w", k_om3w<nn, BA_OM3W_LAB_DIAG, true>);
        OM3W_CASE(5) OM3W_CASE(6) OM3W_CASE(7) OM3W_CASE(8) OM3W_CASE(9) OM3W_CASE(10)
        OM3W_CASE(11) OM3W_CASE(12) OM3W_CASE(13) OM3W_CASE(14)
#undef OM3W_CASE
        default: return hipErrorInvalidValue;
    }
}

}  // namespace ba
