// A stand-alone driver for the host sanitizers (tests/test_sched_cpu.py builds it together with sched_cpu.cpp under
// -fsanitize=address,undefined and runs it): the shadow-queue placement (trt_sched.h) as the pass loop uses it.  For N from 0 to 48 and at
// the sizes of a full pass (2^31 - 2^16, 2^32 - 1, 2^40) a pass is played through: queue lengths that shrink by a fixed sequence, every
// bounce placed against the interval the bounce before left, its records "written" into a byte map of the N slots (small N) that marks who
// may still be reading them.  A write onto a slot still being read without `wait`, an interval outside [0, N), or a `wait` over disjoint
// intervals counts as bad.  Prints "ok <cases>" and returns 0.
#include <cstdint>
#include <cstdio>
#include <vector>

extern "C" void sched_place(uint64_t n, const uint64_t* N, const uint32_t* parity, const uint64_t* prev_at, const uint64_t* prev_n, const uint64_t* cap, uint64_t* at, uint8_t* wait);

namespace {
uint64_t next(uint64_t& state)
{
    state += 0x9E3779B97F4A7C15ull;
    uint64_t z = state;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
}  // namespace

int main()
{
    int cases = 0, bad = 0;
    std::vector<uint64_t> sizes;
    for (uint64_t n = 0; n <= 48; ++n) sizes.push_back(n);
    for (uint64_t n : {0x7FFF0000ull, 0xFFFFFFFFull, 1ull << 40}) sizes.push_back(n);
    uint64_t state = 0x5C4ED;
    for (uint64_t N : sizes)
        for (int keep = 1; keep <= 10; ++keep) {  // tenths of the paths that survive a bounce
            std::vector<uint8_t> reading(N <= 48 ? N : 0, 0);
            uint64_t n_active = N, prev_at = 0, prev_n = 0;
            for (uint32_t b = 0; b < 24; ++b) {
                uint64_t at = 0;
                uint8_t wait = 0;
                const uint32_t parity = b & 1u;
                sched_place(1, &N, &parity, &prev_at, &prev_n, &n_active, &at, &wait);
                ++cases;
                bad += at > N || n_active > N - at;
                const bool meet = prev_n && n_active && at < prev_at + prev_n && prev_at < at + n_active;
                bad += meet != (wait != 0);
                if (wait) for (uint8_t& r : reading) r = 0;  // the walk before is through
                for (uint64_t k = 0; k < n_active && !reading.empty(); ++k) bad += reading[at + k] != 0;
                for (uint8_t& r : reading) r = 0;            // ... and so is the one before it, whose event every bounce waits for
                const uint64_t n_s = n_active ? next(state) % (n_active + 1) : 0;  // the longest shadow queue of the bounce
                for (uint64_t k = 0; k < n_s && !reading.empty(); ++k) reading[at + k] = 1;
                prev_at = at;
                prev_n = n_s;
                n_active = n_active / 10 * keep + (n_active % 10) * keep / 10;
            }
        }
    // more records asked for than the arrays hold: clamped, never outside
    {
        const uint64_t N = 7, prev_at = 0, prev_n = 7, cap = 1000;
        for (uint32_t parity = 0; parity < 2; ++parity) {
            uint64_t at = 99;
            uint8_t wait = 0;
            sched_place(1, &N, &parity, &prev_at, &prev_n, &cap, &at, &wait);
            ++cases;
            bad += at != 0 || !wait;
        }
    }
    std::printf("%s %d\n", bad ? "FAILED" : "ok", cases);
    return bad ? 1 : 0;
}
