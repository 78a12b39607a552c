// gmr_tracker_policy_bwd_plan.h -- the host's plan of the backward pass through the motion tracker's two networks
// (gmr_tracker_policy_bwd.hip): the row chunks, the tile table of the weight-gradient launch, the place of every
// tensor's partial sums in the workspace and the LDS of the sweep.  Asks nothing of the HIP runtime, so that
// tests/cpp/policy_bwd_plan_check.cpp drives it under plain g++ with a gmr_fail of its own, as gmr_tracker_policy_plan.h is driven.
#ifndef GMR_TRACKER_POLICY_BWD_PLAN_H
#define GMR_TRACKER_POLICY_BWD_PLAN_H
#include <stddef.h>
#include <stdint.h>

#include "../../include/gmr_hip.h"
#include "gmr_internal.h"
#include "gmr_tracker_policy_plan.h"

namespace gmr {

constexpr int PBW_TILE = 64;                // a wavefront's block of dW: 2 x 2 accumulator tiles of 32 x 32
// the widest network: 512 inputs in eight tiles by four, three times four by four, one row of four for the last layer
constexpr int PBW_MAX_TILES = (GMR_POLICY_MAX_IN / PBW_TILE) * (GMR_POLICY_MAX_WIDTH / PBW_TILE) +
                              (GMR_POLICY_MAX_HIDDEN - 1) * (GMR_POLICY_MAX_WIDTH / PBW_TILE) * (GMR_POLICY_MAX_WIDTH / PBW_TILE) + GMR_POLICY_MAX_WIDTH / PBW_TILE;
static_assert(GMR_POLICY_BWD_CHUNK % 32 == 0 && GMR_POLICY_BWD_CHUNK >= 32, "a chunk is a whole number of sweep tiles");

// one wavefront's work on one row chunk: dW_layer[j0 .. j0 + 63][i0 .. i0 + 63], and db_layer[j0 .. j0 + 63] where bias is set (i0 = 0)
struct PolicyBwdTile {
  int32_t layer, j0, i0, bias;
};

// one network: where the partial sums of its tensors lie inside a chunk's record, in floats (W_l at 2 l, b_l at 2 l + 1)
struct PolicyBwdNet {
  int32_t tiles = 0;                        // entries of its tile table
  int64_t elems = 0;                        // floats of a chunk's record: every dW and every db
  int64_t off[2 * (GMR_POLICY_MAX_HIDDEN + 1)] = {};
  int32_t stride[2] = {};                   // floats per row of the two LDS buffers of the sweep: g_l lives in buffer l & 1, l = 1 .. L
  size_t lds = 0;
};

struct PolicyBwdPlan {
  int64_t max_rows = 0;
  int32_t chunks = 0;                       // of max_rows
  PolicyBwdNet actor, critic;
  size_t o_part = 0, o_tab_actor = 0, o_tab_critic = 0;      // offsets into the block, each on 256 bytes
  size_t bytes = 0;                         // of the block
};

inline int64_t policy_bwd_chunks(int64_t rows) { return (rows + GMR_POLICY_BWD_CHUNK - 1) / GMR_POLICY_BWD_CHUNK; }

// The tile table and the record of one network; tiles may be null.  The tiles of a layer follow one another with i0 fastest, so that
// the four wavefronts of a workgroup read the same columns of g.
inline void policy_bwd_net(const PolicyShape& s, PolicyBwdNet* n, PolicyBwdTile* tiles) {
  *n = PolicyBwdNet{};
  int w[2] = {0, 0};
  for (int l = 0; l <= s.L; l++) {
    const int K = s.width[l], N = s.width[l + 1];
    n->off[2 * l] = n->elems;
    n->elems += (int64_t)N * K;
    n->off[2 * l + 1] = n->elems;
    n->elems += N;
    for (int j0 = 0; j0 < N; j0 += PBW_TILE)
      for (int i0 = 0; i0 < K; i0 += PBW_TILE) {
        if (tiles) tiles[n->tiles] = PolicyBwdTile{l, j0, i0, i0 == 0 ? 1 : 0};
        n->tiles++;
      }
    if (l >= 1 && N > w[l & 1]) w[l & 1] = N;
  }
  // a row is as long as the widest g_l it ever holds (the last one's 1 .. 32 columns up to a multiple of four) plus four floats, as in the forward
  n->stride[0] = ((w[0] + 3) & ~3) + 4;
  n->stride[1] = ((w[1] + 3) & ~3) + 4;
  n->lds = (size_t)GMR_POLICY_TILE * (size_t)(n->stride[0] + n->stride[1]) * sizeof(float);
}

// The block of a set_backward call: the partial sums of the larger network for every chunk of max_rows, then the two tile tables.
inline int policy_bwd_plan(const PolicyShape& actor, const PolicyShape& critic, int64_t max_rows, PolicyBwdPlan* p) {
  if (max_rows < 1 || max_rows > GMR_POLICY_BWD_MAX_ROWS)
    return gmr_fail(GMR_ERR_ARG, "max_rows = %lld, 1 .. GMR_POLICY_BWD_MAX_ROWS = %d are taken", (long long)max_rows, GMR_POLICY_BWD_MAX_ROWS);
  *p = PolicyBwdPlan{};
  p->max_rows = max_rows;
  p->chunks = (int32_t)policy_bwd_chunks(max_rows);
  policy_bwd_net(actor, &p->actor, nullptr);
  policy_bwd_net(critic, &p->critic, nullptr);
  const int64_t elems = p->actor.elems > p->critic.elems ? p->actor.elems : p->critic.elems;
  auto take = [&](size_t bytes) {
    const size_t at = p->bytes;
    p->bytes += (bytes + 255) / 256 * 256;
    return at;
  };
  p->o_part = take((size_t)p->chunks * (size_t)elems * sizeof(float));
  p->o_tab_actor = take((size_t)p->actor.tiles * sizeof(PolicyBwdTile));
  p->o_tab_critic = take((size_t)p->critic.tiles * sizeof(PolicyBwdTile));
  return GMR_OK;
}

}  // namespace gmr
#endif
