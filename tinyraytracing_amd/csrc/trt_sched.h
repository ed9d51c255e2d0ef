// Where a bounce's shadow records go, and whether the k_shade that writes them has to wait for the shadow walk of the bounce before
// (DESIGN.md §4.3).  Plain C++, no HIP: the host loop of trt_api.hip calls it, tests/sched/sched_cpu.cpp builds it for the CPU.
//
// A light's shadow queue is three arrays of N records (N = paths of the pass).  k_shade of bounce b emits at most cap = n_active(b) records
// per light, from the pointer it is given upward.  Bounces take the two ends of the arrays in turn: an even bounce writes [0, cap), an odd
// one [N - cap, N).  The shadow walk of bounce b - 1, which may still be running on the side stream, reads [prev_at, prev_at + prev_n) of
// the other end (prev_n: the longest of its lights' queues).  Where the two intervals are disjoint, k_shade of bounce b needs no order
// against that walk; where they meet, it waits for it, which is the order of a single stream.
#pragma once
#include <cstdint>

struct ShadowPlace {
    uint64_t at;  // first record k_shade writes: the offset of the ShadowQueue pointers
    bool wait;    // the write interval [at, at + cap) meets the interval being read
};

inline ShadowPlace shadowPlace(uint64_t N, uint32_t parity, uint64_t prev_at, uint64_t prev_n, uint64_t cap)
{
    if (cap > N) cap = N;  // (the host loop never asks for more: n_active <= N)
    ShadowPlace p;
    p.at = (parity & 1u) ? N - cap : 0u;
    p.wait = prev_n != 0u && cap != 0u && p.at < prev_at + prev_n && prev_at < p.at + cap;
    return p;
}
