// The tanh-normal policy head, one action dimension at a time (`NormalTanhDistribution` [UP brax.training.distribution]): from the
// location logit `loc`, the pre-softplus scale logit `s` and one standard-normal draw `eps`,
//   scale = softplus(s) + min_std,  raw = loc + scale * eps,  action = tanh(raw),
//   log_prob term = -0.5 z^2 - log scale - 0.5 log 2 pi - log|d tanh(raw) / d raw|,  z = (raw - loc) / scale,
//   log|d tanh(x) / dx| = 2 (log 2 - x - softplus(-2 x)).
// Every site that samples or scores an action calls these: the actor inside the step kernel (rr_actor_step, csrc/rr_kernel.h), the
// two-launch actor's tail and rr_policy_sample_kernel, and the learner's rr_ppo_loss_kernel (csrc/rr_ppo.h).  The PPO ratio is
// exp(log_prob under the learner - log_prob under the actor), so the two sides must round alike: z is formed from raw (not taken as
// eps), and the division is the IEEE one.
#pragma once
#include <hip/hip_runtime.h>

constexpr float RR_HALF_LOG_2PI = 0.91893853320467274178f, RR_LOG2 = 0.69314718055994530942f;

static __device__ __forceinline__ float rr_softplus(float x) { return fmaxf(x, 0.0f) + log1pf(expf(-fabsf(x))); }
static __device__ __forceinline__ float rr_tn_scale(float s, float min_std) { return rr_softplus(s) + min_std; }
static __device__ __forceinline__ float rr_tn_raw(float loc, float scale, float eps) { return loc + scale * eps; }
static __device__ __forceinline__ float rr_tn_log_det(float x) { return 2.0f * (RR_LOG2 - x - rr_softplus(-2.0f * x)); }
// log-prob term of one action dimension: the action tanh(raw) under the head (loc, scale)
static __device__ __forceinline__ float rr_tn_logp(float loc, float scale, float raw) {
  const float z = (raw - loc) / scale;
  return -0.5f * z * z - logf(scale) - RR_HALF_LOG_2PI - rr_tn_log_det(raw);
}
// entropy term of one action dimension, estimated at the sample x = rr_tn_raw(loc, scale, eps)
static __device__ __forceinline__ float rr_tn_entropy(float scale, float x) { return 0.5f + RR_HALF_LOG_2PI + logf(scale) + rr_tn_log_det(x); }
