// mgn_status.h -- how an entry point of the C ABI reports a refusal or a HIP
// error, for the units that define entry points beside their kernels
// (mgn_rnorm.hip, mgn_tear.hip, mgn_xbuf.hip, mgn_pbuf.hip).  Defined in
// mgn_api.hip, where mgn_env is complete and the thread-local error string
// behind mgn_global_error() lives.
#pragma once

#include <hip/hip_runtime.h>

#include <string>

#include "../../include/madigan_amd.h"

namespace mgn {

// records msg as the handle's (e may be null) and the thread's last error; returns code
int fail(mgn_env* e, int code, const std::string& msg);

// MGN_OK, or MGN_ERR_DEVICE with "<what>: <HIP's error string>" recorded
int check_hip(mgn_env* e, hipError_t st, const char* what);

}  // namespace mgn
