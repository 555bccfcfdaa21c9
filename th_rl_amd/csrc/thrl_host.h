// thrl_host.h -- host helpers shared by the two files of the extern "C" surface: thrl_api.hip (the ABI, the training
// plans, the run functions, the ops / nn / cac wrappers) defines them, thrl_api_analysis.hip (the post-training
// analyses) calls them.  Internal: nothing here is exported through include/thrl.h.
#pragma once
#include "thrl_device.h"

namespace thrl::host {

// Sets the calling thread's thrl_last_error() text (one thread-local string, in thrl_api.hip) and returns code.
int fail(int code, const char* fmt, ...);
int hip_fail(int e, const char* what);

// the checks every entry point makes on its config
int validate(const thrl_cfg* c);
void fill_agents(const thrl_cfg* c, AgentParams* ag, EnvParams* env);
// rows reachable after a transition, per agent [lo, hi]
void reach_window(const thrl_cfg* c, int* lo, int* hi);

// host restatements of the device's scale_action and encode64, operation for operation
double h_scale(int k, const thrl_cfg* c, int i);
int h_encode64(double price, const thrl_cfg* c, int i);

}  // namespace thrl::host
