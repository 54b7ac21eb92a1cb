// How the host units of librcw_hip report a failure: fail() leaves the text that rcw_last_error hands out and returns the RCW_ERR_* code it
// was given.  Declarations and the two macros only: the definitions, and the thread's buffer, are rcw_api.hip's, next to rcw_last_error.
#pragma once
#include "../../include/rcw.h"

#include <hip/hip_runtime.h>

int fail(int code, const char* fmt, ...);
#ifdef RCW_DEV_SWITCHES
// Development build only: which error returns has the process taken?  Every `fail(...)` of a unit leaves its source file and line in a
// table that rcw_dev_fail_sites hands out, a unit at a time (tests: which refusals does the suite provoke, which never).  No header holds
// such a site: RCW_HIP's is where the macro is used.
int fail_at(const char* file, int line, int code, const char* fmt, ...);
#define fail(...) fail_at(__FILE_NAME__, __LINE__, __VA_ARGS__)
#endif

// The text of a failed runtime call, which is thereby REPORTED: the runtime also keeps the code as the thread's last error, and the launchers'
// hipGetLastError() would hand it out as their own (a create that ran out of memory made the next rcw_create fail in its first launch).
const char* hip_failure(hipError_t e);
int hip_code(hipError_t e);   // the RCW_ERR_* of a failed runtime call

#define RCW_HIP(expr)                                                                   \
    do {                                                                                \
        hipError_t e_ = (expr);                                                         \
        if (e_ != hipSuccess)                                                           \
            return fail(hip_code(e_), "%s failed: %s", #expr, hip_failure(e_));         \
    } while (0)
