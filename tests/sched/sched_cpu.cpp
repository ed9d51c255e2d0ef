// CPU build of the shadow-queue placement (tinyraytracing_amd/csrc/trt_sched.h), for tests/test_sched_cpu.py and tests/sched/sched_san.cpp:
// the function itself over arrays of cases, so that a sweep is one call.
#include <stdint.h>

#include "trt_sched.h"

extern "C" {

// case k: shadowPlace(N[k], parity[k], prev_at[k], prev_n[k], cap[k]) -> at[k], wait[k]
void sched_place(uint64_t n, const uint64_t* N, const uint32_t* parity, const uint64_t* prev_at, const uint64_t* prev_n, const uint64_t* cap, uint64_t* at, uint8_t* wait)
{
    for (uint64_t k = 0; k < n; ++k) {
        const ShadowPlace p = shadowPlace(N[k], parity[k], prev_at[k], prev_n[k], cap[k]);
        at[k] = p.at;
        wait[k] = p.wait ? 1 : 0;
    }
}

}  // extern "C"
