// ba_wave3t.hip -- WAVE engine, effective depth 3 with the wave-shared pair
// table (k_om3wt; its own translation unit so it compiles beside k_om3w).
#include "ba_wave.hpp"

namespace ba {

// n = 10, the only tree k_om3wt is compiled for (launch_wave_engine, ba_wave3.hip)
hipError_t launch_wave3t(const RunArgs& a) {
    return launch_wave<Om3WT<10>>(a, k_om3wt<10>, "k_om3wt", k_om3wt<10, true>);
}

}  // namespace ba
