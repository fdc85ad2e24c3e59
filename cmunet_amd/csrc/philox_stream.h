// philox_stream.h -- the counter-based random stream of the device samplers (genesis.hip, ft_augment.hip, moco_views.hip) and the
// 53-bit uniform laws on raw Philox words.  One copy: "the same (seed, offset) gives the same bits" is every trainer's contract.
#pragma once
#include "common.h"

// two 32-bit words -> uniform double on 53 bits: [0, 1) as random.random() ...
__device__ static inline double philox_u53(uint32_t hi, uint32_t lo) {
    return (double)((((uint64_t)hi << 32) | lo) >> 11) * (1.0 / 9007199254740992.0);
}
// ... and its half-open sibling that is never 0, the argument of Box-Muller's log
__device__ static inline double philox_u53_open(uint32_t hi, uint32_t lo) {
    return ((double)((((uint64_t)hi << 32) | lo) >> 11) + 0.5) * (1.0 / 9007199254740992.0);
}

// stream id (counter word c1) of a per-record stream: purpose << 28 | record (genesis.hip packs image and block instead: gen_id)
__device__ static inline uint32_t philox_id(int purpose, int rec) { return ((uint32_t)purpose << 28) | (uint32_t)rec; }

// one stream: c0 counts the refills, c1 = id, (c2, c3) = offset, key = seed; four words per Philox4x32-10 call, handed out in order
struct PhiloxStream {
    uint32_t k0, k1, id, o0, o1, c0;
    uint32_t buf[4];
    int pos;
    __device__ PhiloxStream(uint64_t seed, uint64_t offset, uint32_t id_)
        : k0((uint32_t)seed), k1((uint32_t)(seed >> 32)), id(id_), o0((uint32_t)offset), o1((uint32_t)(offset >> 32)), c0(0), pos(4) {}
    __device__ uint32_t next() {
        if (pos == 4) {
            philox4x32_10(c0++, id, o0, o1, k0, k1, buf);
            pos = 0;
        }
        return buf[pos++];
    }
    // random.random(): uniform double in [0, 1) on 53 bits
    __device__ double uniform() {
        const uint32_t hi = next(), lo = next();
        return philox_u53(hi, lo);
    }
    // random.uniform(a, b) = a + (b - a) * random(), each operation rounded on its own
    __device__ double uniform(double a, double b) { return __dadd_rn(a, __dmul_rn(__dadd_rn(b, -a), uniform())); }
    // uniform integer in [0, n), n >= 1: Lemire's multiply-shift with rejection (exactly uniform)
    __device__ uint32_t below(uint32_t n) {
        uint64_t m = (uint64_t)next() * n;
        uint32_t l = (uint32_t)m;
        if (l < n) {
            const uint32_t t = (0u - n) % n;
            while (l < t) {
                m = (uint64_t)next() * n;
                l = (uint32_t)m;
            }
        }
        return (uint32_t)(m >> 32);
    }
    __device__ int randint(int a, int b) { return a + (int)below((uint32_t)(b - a + 1)); }   // random.randint: both ends included
};
