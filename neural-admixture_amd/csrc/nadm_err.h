// The per-thread error message behind nadm_last_error(): plain C++, no HIP header, so that the host-only units
// (nadm_host_io.cpp, nadm_layout.cpp, nadm_gmm.cpp, nadm_passes_host.cpp) build with any C++ compiler.
#pragma once
#include <stdio.h>
#include <string.h>
#include <math.h>
#include "../../include/nadm.h"

namespace nadm {

inline char* err_buf() {
    static thread_local char buf[512] = {0};
    return buf;
}
inline int fail(const char* msg) {
    snprintf(err_buf(), 512, "%s", msg);
    return 1;
}

}  // namespace nadm
