// gmr_terrain.h -- the terrain lookup of a motion tracker: ONE definition for gmr_tracker_feet.hip (terrain heights,
// feet) and gmr_tracker_episode.hip (reset states).  Include it after the translation unit's "#pragma clang fp contract(off)": every
// operation is rounded once.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "gmr_handles.h"

namespace gmr {

// Terrain.terrain_heights (terrain.py:105-118) at one point, in the reference's NumPy promotion: the pixel coordinate in float32, the
// weights, the four products, their sum and the vertical scale in float64, one rounding to float32.  Each of the four indices is clamped to
// the field and the weights stay as computed; *outside says whether one was clamped or the coordinate is not finite (then the height is NaN).
__device__ __forceinline__ float terrain_height(const TerrainTables& T, float px, float py, bool* outside) {
  *outside = false;
  if (!T.field) return 0.0f;
  const float x = T.border + __fdiv_rn(px, T.hs), y = T.border + __fdiv_rn(py, T.hs);                       // :105-106
  if (!(fabsf(x) <= 3.4028234663852886e38f) || !(fabsf(y) <= 3.4028234663852886e38f)) {
    *outside = true;
    return __builtin_nanf("");
  }
  const double xd = (double)x, yd = (double)y;
  const double x1 = (double)floorf(x), y1 = (double)floorf(y), x2 = x1 + 1.0, y2 = y1 + 1.0;               // :107-110
  const double mx = (double)(T.nx - 1), my = (double)(T.ny - 1);
  *outside = x1 < 0.0 || x2 > mx || y1 < 0.0 || y2 > my;
  const size_t ix1 = (size_t)fmin(fmax(x1, 0.0), mx), ix2 = (size_t)fmin(fmax(x2, 0.0), mx);
  const size_t iy1 = (size_t)fmin(fmax(y1, 0.0), my), iy2 = (size_t)fmin(fmax(y2, 0.0), my);
  const size_t ny = (size_t)T.ny;
  const double h11 = (double)T.field[ix1 * ny + iy1], h21 = (double)T.field[ix2 * ny + iy1];
  const double h12 = (double)T.field[ix1 * ny + iy2], h22 = (double)T.field[ix2 * ny + iy2];
  const double wx2 = x2 - xd, wx1 = xd - x1, wy2 = y2 - yd, wy1 = yd - y1;
  const double s = ((wx2 * wy2 * h11 + wx1 * wy2 * h21) + wx2 * wy1 * h12) + wx1 * wy1 * h22;             // :113-116
  return (float)(s * T.vs);                                                                               // :118-119
}

}  // namespace gmr
