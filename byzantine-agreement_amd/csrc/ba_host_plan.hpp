// ba_host_plan.hpp -- the chunk and staging arithmetic of the protocols' host
// entries (host_run, ba_api.cpp).  Plain C++ with no HIP in it, so a stand-alone
// program can run it under a host sanitizer.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

namespace ba {

// How one host run cuts its batch and lays out the ctx's staging buffers:
//   io_dec  [chunk] decisions (8 B), then the extra plane if it rides behind them
//   io_out  [chunk] outcome bytes, then the extra plane if it rides behind them
// A buffer is sized for both planes as soon as either is asked for, so the extra
// plane's place does not depend on whether the primary one is wanted.
struct HostPlan {
    uint64_t chunk = 0;                    // trials per chunk, <= batch
    size_t dec_bytes = 0, out_bytes = 0;   // 0: the buffer is not used
    size_t extra_off = 0;                  // the extra plane's byte offset in its buffer
};

// dflt: the chunk without an override; env: the value of the tests' chunk
// variable or NULL (rounded down to a multiple of 64, ignored when that is 0).
// extra_elem: bytes per trial of the protocol's extra plane, 0 when it has none;
// extra_behind_dec: it rides in io_dec, else in io_out.
inline HostPlan host_plan(uint64_t batch, uint64_t dflt, const char* env, bool want_dec,
                          bool want_out, bool want_extra, size_t extra_elem, bool extra_behind_dec) {
    HostPlan h;
    h.chunk = dflt;
    if (env) {
        const uint64_t c = strtoull(env, nullptr, 0) & ~63ull;
        if (c) h.chunk = c;
    }
    if (h.chunk > batch) h.chunk = batch;
    const size_t dec_elem = 8 + (extra_behind_dec ? extra_elem : 0);
    const size_t out_elem = 1 + (extra_behind_dec ? 0 : extra_elem);
    if (want_dec || (want_extra && extra_behind_dec)) h.dec_bytes = h.chunk * dec_elem;
    if (want_out || (want_extra && !extra_behind_dec)) h.out_bytes = h.chunk * out_elem;
    h.extra_off = h.chunk * (extra_behind_dec ? 8 : 1);
    return h;
}

// trials of the chunk that starts at trial t0
inline uint64_t chunk_trials(uint64_t batch, uint64_t t0, uint64_t chunk) {
    return batch - t0 < chunk ? batch - t0 : chunk;
}

}  // namespace ba
