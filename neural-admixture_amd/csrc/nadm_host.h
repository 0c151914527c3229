// nadm_host_rules.h + what needs the HIP runtime: for the units that launch kernels.
#pragma once
#include <hip/hip_runtime.h>
#include "nadm_host_rules.h"

namespace nadm {

inline int check_launch(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        snprintf(err_buf(), 512, "%s: launch failed: %s", what, hipGetErrorString(e));
        return 2;
    }
    return 0;
}

}  // namespace nadm
