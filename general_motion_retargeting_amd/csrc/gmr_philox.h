// gmr_philox.h -- Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11): a
// counter-based generator, so a draw depends on its (counter, key) alone -- not on the launch shape, not on the order in
// which environments are served -- and tests/tracker_mirror.py reproduces it word for word.  Plain integer C++: the motion
// tracker's kernels (gmr_tracker.hip) and, under g++, tests/cpp/philox_check.cpp compile the same lines.
#ifndef GMR_PHILOX_H
#define GMR_PHILOX_H
#include <stdint.h>

#ifdef __HIPCC__
#define GMR_PHILOX_FN __host__ __device__ __forceinline__
#else
#define GMR_PHILOX_FN inline
#endif

namespace gmr {

// out[0..3] = Philox4x32-10(counter c[0..3], key k[0..1])
GMR_PHILOX_FN void philox4x32(const uint32_t c[4], const uint32_t k[2], uint32_t out[4]) {
  uint32_t c0 = c[0], c1 = c[1], c2 = c[2], c3 = c[3], k0 = k[0], k1 = k[1];
  for (int r = 0; r < 10; r++) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// word 1 of a draw -> u in [0, 1): 24 bits, exact in float32
GMR_PHILOX_FN float philox_unit(uint32_t w) { return (float)(w >> 8) * 5.9604644775390625e-8f; }

// a word -> u in (0, 1]: 24 bits, exact in float32; what a logarithm may take
GMR_PHILOX_FN float philox_unit_open(uint32_t w) { return (float)((w >> 8) + 1u) * 5.9604644775390625e-8f; }

// word 0 of a draw -> one of C equally likely clips
GMR_PHILOX_FN int philox_below(uint32_t w, int C) { return (int)(((uint64_t)w * (uint64_t)C) >> 32); }

}  // namespace gmr
#endif
