// The Philox4x32-10 of csrc/gmr_philox.h, compiled for the host by g++, against the known-answer vectors of the Random123
// distribution; prints the three outputs (tests/test_motion_tracker_host.py compares them) and the two conversions at their edges.
#include <cstdio>

#include "../../general_motion_retargeting_amd/csrc/gmr_philox.h"

int main() {
  const uint32_t ctr[3][4] = {{0, 0, 0, 0},
                              {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu},
                              {0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u}};
  const uint32_t key[3][2] = {{0, 0}, {0xffffffffu, 0xffffffffu}, {0xa4093822u, 0x299f31d0u}};
  for (int i = 0; i < 3; i++) {
    uint32_t w[4];
    gmr::philox4x32(ctr[i], key[i], w);
    std::printf("%08x %08x %08x %08x\n", w[0], w[1], w[2], w[3]);
  }
  std::printf("%.9g %.9g %d %d\n", (double)gmr::philox_unit(0u), (double)gmr::philox_unit(0xffffffffu), gmr::philox_below(0u, 7),
              gmr::philox_below(0xffffffffu, 7));
  return 0;
}
