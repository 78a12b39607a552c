// gmr_tracker_policy_plan.h -- the shapes of the motion tracker's two networks (gmr_tracker_policy.hip) as the host
// checks them and lays them out: the capacities of include/gmr_hip.h N17, the order of the parameter list and the two activation buffers
// a workgroup keeps in LDS.  Asks nothing of the HIP runtime, so that tests/cpp/policy_plan_check.cpp drives it under plain g++ with a
// gmr_fail of its own, as gmr_tracker_host.h is driven.
#ifndef GMR_TRACKER_POLICY_PLAN_H
#define GMR_TRACKER_POLICY_PLAN_H
#include <stddef.h>
#include <stdint.h>

#include "../../include/gmr_hip.h"
#include "gmr_internal.h"

namespace gmr {

// one network: width[0] the input, width[1 .. L] the hidden layers, width[L + 1] the output
struct PolicyShape {
  int32_t L = 0;
  int32_t width[GMR_POLICY_MAX_HIDDEN + 2] = {};
  int32_t first = 0;                        // where its (W, b) pairs start in the parameter list
  int32_t stride[2] = {};                   // floats per row of the two LDS buffers: layer l reads buffer l & 1 and writes the other
  size_t lds = 0;                           // bytes of both buffers
};

// the input of the first layer in LDS: up to the next multiple of the eight k of one operand load, the rest zeros
inline int policy_padded(int in) { return (in + 7) & ~7; }

// The buffers of one network: a row is as long as the widest layer it ever holds plus four floats, so that rows stay on sixteen bytes
// and consecutive rows start sixteen bytes further round the banks.
inline void policy_layout(PolicyShape& s) {
  int w[2] = {policy_padded(s.width[0]), 0};
  for (int l = 1; l <= s.L; l++)
    if (s.width[l] > w[l & 1]) w[l & 1] = s.width[l];
  s.stride[0] = w[0] + 4;
  s.stride[1] = w[1] + 4;
  s.lds = (size_t)GMR_POLICY_TILE * (size_t)(s.stride[0] + s.stride[1]) * sizeof(float);
}

inline int policy_hidden_check(const char* net, int n, const int* hidden) {
  if (n < 1 || n > GMR_POLICY_MAX_HIDDEN) return gmr_fail(GMR_ERR_ARG, "%s: %d hidden layers, 1 .. %d are taken", net, n, GMR_POLICY_MAX_HIDDEN);
  if (!hidden) return gmr_fail(GMR_ERR_ARG, "%s: null hidden widths", net);
  for (int l = 0; l < n; l++)
    if (hidden[l] < GMR_POLICY_WIDTH_STEP || hidden[l] > GMR_POLICY_MAX_WIDTH || hidden[l] % GMR_POLICY_WIDTH_STEP)
      return gmr_fail(GMR_ERR_ARG, "%s: hidden[%d] = %d, a multiple of %d in %d .. %d is needed", net, l, hidden[l], GMR_POLICY_WIDTH_STEP, GMR_POLICY_WIDTH_STEP,
                      GMR_POLICY_MAX_WIDTH);
  return GMR_OK;
}

// The two networks of a set_policy call, checked: the parameter list is logstd, the critic's (W, b) pairs, the actor's (W, b) pairs.
inline int policy_plan(int obs_cols, int priv_cols, int act_cols, int n_actor, const int* actor_hidden, int n_critic, const int* critic_hidden,
                       PolicyShape* actor, PolicyShape* critic) {
  if (obs_cols < 1 || priv_cols < 0 || obs_cols > GMR_POLICY_MAX_IN || priv_cols > GMR_POLICY_MAX_IN || obs_cols + priv_cols > GMR_POLICY_MAX_IN)
    return gmr_fail(GMR_ERR_ARG, "obs_cols = %d and priv_cols = %d: obs_cols at least 1, priv_cols at least 0 and at most %d together are taken", obs_cols, priv_cols,
                    GMR_POLICY_MAX_IN);
  if (act_cols < 1 || act_cols > GMR_LOSS_MAX_ACT) return gmr_fail(GMR_ERR_ARG, "act_cols = %d, 1 .. GMR_LOSS_MAX_ACT = %d are taken", act_cols, GMR_LOSS_MAX_ACT);
  int rc = policy_hidden_check("actor", n_actor, actor_hidden);
  if (rc != GMR_OK) return rc;
  rc = policy_hidden_check("critic", n_critic, critic_hidden);
  if (rc != GMR_OK) return rc;
  *actor = PolicyShape{};
  *critic = PolicyShape{};
  critic->L = n_critic;
  critic->width[0] = obs_cols + priv_cols;
  for (int l = 0; l < n_critic; l++) critic->width[l + 1] = critic_hidden[l];
  critic->width[n_critic + 1] = 1;
  critic->first = 1;
  actor->L = n_actor;
  actor->width[0] = obs_cols;
  for (int l = 0; l < n_actor; l++) actor->width[l + 1] = actor_hidden[l];
  actor->width[n_actor + 1] = act_cols;
  actor->first = 1 + 2 * (n_critic + 1);
  policy_layout(*actor);
  policy_layout(*critic);
  return GMR_OK;
}

// tensors in the parameter list of two networks
inline int policy_tensors(const PolicyShape& actor, const PolicyShape& critic) { return 1 + 2 * (critic.L + 1) + 2 * (actor.L + 1); }

}  // namespace gmr
#endif
