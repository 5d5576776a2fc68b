// lbk8s_env_steps.hip — lbk8s_env.hip and lbk8s_steps.hip compiled as one unit.
//
// The one-launch step kernels (lbk8s_steps.h) instantiate the slice layout's device functions
// for W = 16, EPL = 1, as k_reset_slice / k_step_slice / k_rollout_slice<16, 1> do.  Compiled in
// a module of their own, those four env kernels come out with other code than next to the step
// kernels (the same instructions in another association and order; k_rollout_slice<16, 1> with
// four more VGPRs), and k_step_slice<16, 1, false> then measured 1.4 % slower at 4096 envs
// (profiles/units_split_ab.json).  The step kernels add 4.5 s to this unit's 36 s.
#include "lbk8s_env.hip"
#include "lbk8s_steps.hip"
